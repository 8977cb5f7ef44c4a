"""Functional pin of the self-defined steerable-pyramid spec (oracle/pyramid_cpu.py) against the reference's TRAINED
PhaseNet weights -- see tools/pyramid_spec_pin.py (the generator) and DESIGN.md section 2.

  * the committed table (tests/golden/pyramid_spec_pin.json) carries the conclusions DESIGN.md draws from it;
  * the oracle still computes the spec the table was measured on (tests/golden/pyramid_spec_fingerprint.npz, written
    with the table), so a change to the oracle's spec fails here until the table is measured again.
"""
import json
import os
import sys

import numpy as np

from conftest import GOLDEN, ROOT


def _rows():
    with open(os.path.join(GOLDEN, "pyramid_spec_pin.json")) as f:
        return {r["variant"]: r for r in json.load(f)["rows"]}


def test_committed_table_supports_the_spec():
    rows = _rows()
    ours = rows["ours: ceil sizes, DC at h//2"]
    # PhaseNet-only beats frame averaging as soon as the motion is not sub-pixel-ish (shifts >= 2 px)
    for s in ours["per_shift"][1:]:
        assert s["psnr_phasenet"] >= s["psnr_average"] + 2.0, s
    # the plausible level-size rules are indistinguishable to the trained network: no reason to leave `ceil`
    for k in ("floor sizes", "round sizes"):
        assert abs(rows[k]["mean_psnr_phasenet"] - ours["mean_psnr_phasenet"]) <= 0.1
    # conventions the network CAN see are pinned: each control loses >= 1.5 dB
    for k in ("control: band order reversed", "control: phase sign flipped", "control: bands rotated +90 deg",
              "control: bands rotated -90 deg", "control: DC at (h-1)//2"):
        assert rows[k]["mean_psnr_phasenet"] <= ours["mean_psnr_phasenet"] - 1.5, k


def test_oracle_spec_is_the_one_the_table_was_measured_on():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import pyramid_spec_pin as pin
    want = np.load(os.path.join(GOLDEN, "pyramid_spec_fingerprint.npz"))
    got = pin.spec_fingerprint()
    assert set(got) == set(want.files)
    for k, v in got.items():
        assert v.shape == want[k].shape, k
        if k.endswith("_shape"):
            assert np.array_equal(v, want[k]), k
        else:
            assert np.abs(v - want[k]).max() <= 1e-4 * max(1e-3, float(np.abs(want[k]).max())), k
