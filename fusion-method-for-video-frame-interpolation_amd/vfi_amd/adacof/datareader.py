"""Vimeo-90k triplet reader of the AdaCoF trainer -- reference src/adacof/datareader.py:15-72, which is the class of
src/train/datareader.py line for line: the one mirror (vfi_amd/train/datareader.py) serves both."""
from ..train.datareader import DBreader_Vimeo90k, TripletLoader, cointoss  # noqa: F401
