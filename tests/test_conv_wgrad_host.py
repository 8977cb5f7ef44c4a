"""The weight gradient's tile walk on the host: the case table of conv_wgrad_ref.py gives the plans it states, and the
modelled walk of splits and tiles covers every pixel exactly once.  No GPU."""
import collections

import pytest
import torch

import conv_wgrad_ref as R


@pytest.mark.parametrize("case,cap", R.CASE_CAPS, ids=R.CASE_CAP_IDS)
def test_plan_gives_the_table(case, cap):
    """A later edit of the table cannot silently fall back to one tile per workgroup: tiles_per_split, splits and the last
    split's tile count are literals in the table."""
    p = R.case_plan(case, cap)
    assert (p.tiles_per_split, p.splits, p.last_tiles) == case.caps[cap], (case.id, cap, p)
    assert p.tiles_total == case.n * p.tiles_x * p.tiles_y
    assert (p.splits - 1) * p.tiles_per_split + p.last_tiles == p.tiles_total and 1 <= p.last_tiles <= p.tiles_per_split
    if cap is not None:
        assert p.splits <= cap
        if p.tiles_total > 1:
            assert p.tiles_per_split > 1, "a cap is in the table to make a workgroup walk several tiles"


def test_table_reaches_what_it_is_there_for():
    plans = [(c, m, R.case_plan(c, m)) for c, m in R.CASE_CAPS]
    per_image = lambda p: p.tiles_x * p.tiles_y
    # a run that crosses an image boundary in its middle, and one that crosses a tile-row end
    assert any(p.tiles_per_split > 1 and per_image(p) % p.tiles_per_split and c.n > 1 for c, m, p in plans)
    assert any(p.tiles_per_split > 1 and p.tiles_x % p.tiles_per_split and p.tiles_x > 1 for c, m, p in plans)
    assert any(1 < p.last_tiles < p.tiles_per_split for c, m, p in plans)                 # a ragged last split of > 1 tile
    assert any(p.splits == 1 and p.tiles_total > 8 for c, m, p in plans)                  # one workgroup walks everything
    assert {c.ks for c, m, p in plans if p.tiles_per_split > 1} == {1, 3, 5}
    assert {"zeros", "reflect"} == {c.pad for c, m, p in plans if p.tiles_per_split > 1}
    assert {p.col_blocks for c, m, p in plans} >= {1, 2, 3} and {p.co_blocks for c, m, p in plans} >= {1, 2, 3}
    # slab_reduce_kernel: slab 0, groups of eight, remainder
    assert {p.splits for c, m, p in plans} >= {1, 2, 9, 10, 17, 18}
    sliced = [(c, m, p) for c, m, p in plans if c.sliced]
    assert len({c.key for c, m, p in sliced}) == 2 and all(c.n == 2 for c, m, p in sliced)
    assert all(any(p.tiles_per_split > 1 for c2, m, p in sliced if c2 is c) for c, _, _ in sliced)


@pytest.mark.parametrize("case", R.CASES, ids=[c.id for c in R.CASES])
def test_walk_covers_every_pixel_once(case):
    for cap in case.caps:
        p = R.case_plan(case, cap)
        seen = collections.Counter()
        per_split = collections.Counter()
        for split, n, y, x in R.walk(p, case.ks, case.h, case.w):
            seen[(n, y, x)] += 1
            per_split[split] += 1
        assert len(seen) == case.n * case.h * case.w and set(seen.values()) == {1}, (case.id, cap)
        assert all(0 <= n < case.n and 0 <= y < case.h and 0 <= x < case.w for n, y, x in seen)
        assert set(per_split) == set(range(p.splits)), "every slab the reduction reads is written"


def test_plan_default_workspace_never_caps_the_table():
    """With the default workspace the split count of every case comes from the tile count alone."""
    for c in R.CASES:
        p = R.case_plan(c, None)
        assert p.splits == p.tiles_total and p.tiles_per_split == 1


@pytest.mark.parametrize("case", R.CASES, ids=[c.id for c in R.CASES])
def test_integer_references_are_exact_in_float32(case):
    """What lets the GPU test ask for torch.equal: with integer data every partial sum of |x||dy| -- hence of any subset of
    the terms, in any order -- stays below 2**24, so fp32 adds and fmas are exact."""
    d = R.data(case.key, "int")
    assert torch.equal(d.dw, d.dw.round()) and torch.equal(d.db, d.db.round())
    assert d.a.max().item() < 2 ** 24 and d.sum_abs_dy.max().item() < 2 ** 24
    assert torch.equal(d.dw.float().double(), d.dw)


def test_float32_cpu_stays_inside_the_bound():
    """The per-element bound (K+1) 2**-24 A of the GPU test, held here by torch's own float32 weight gradient."""
    worst = 0.0
    for c in R.CASES:
        d = R.data(c.key, "randn")
        x, dy = d.x.clone(), d.dy
        w32 = torch.zeros((c.cout, c.cin, c.ks, c.ks), requires_grad=True)
        (R._pad_conv(x, w32, c.pad) * dy).sum().backward()
        err = (w32.grad.double() - d.dw).abs()
        assert (err <= (d.k + 1) * 2.0 ** -24 * d.a).all(), c.id
        worst = max(worst, (err / (2.0 ** -24 * d.a).clamp_min(1e-300)).max().item())
    print("float32 torch on the CPU: worst err / (2^-24 A) = %.2f" % worst)
