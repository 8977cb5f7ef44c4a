"""The scene-cut rule of the clip loop (interpolate_stream), on the host and without torch: what the
loop hands to the device, and the same rule in the units a user sets.

With `sad` the sum of absolute luma differences of two consecutive frames of n luma bytes, the mean absolute difference
in percent is m = 100 sad / (255 n); the score of a pair is min(m, |m - m_prev|) with m_prev = 0 for the first pair, and a
pair is a cut when score >= threshold.  This is the rule ffmpeg's scdet filter documents; nothing here was compared with
ffmpeg.  The device decides on integers: score >= threshold  <=>  min(sad, |sad - sad_prev|) >= min_sad(threshold, n).
"""
from fractions import Fraction
import math


def min_sad(threshold, n):
    """The smallest integer s with 100 s / (255 n) >= threshold: ceil(threshold * 255 * n / 100), in exact arithmetic on the
    threshold's shortest decimal form (0.1 is one tenth, not the float next to it).  threshold <= 0 gives 0: every pair is
    a cut."""
    n = int(n)
    if n <= 0:
        raise ValueError(f"scene.min_sad: bad size {n}")
    t = float(threshold)
    if not math.isfinite(t):
        raise ValueError(f"scene.min_sad: threshold {threshold!r} is not finite")
    return max(0, math.ceil(Fraction(repr(t)) * 255 * n / 100))


def score(sad, sad_prev, n):
    """min(m, |m - m_prev|) in percent; sad_prev None for the first pair."""
    s, p = int(sad), (0 if sad_prev is None else int(sad_prev))
    return 100.0 * min(s, abs(s - p)) / (255.0 * int(n))
