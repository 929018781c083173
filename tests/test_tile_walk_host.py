"""The restated tile walks (tests/tile_walk.py) and the cases of tests/test_gpu_tile_walk.py, on the CPU: each walk visits every tile
once, three mutants of the restatement do not, the cases have the properties they are there for at 256 CUs, and the f32 oracle's
noise against its f64 run stays below the 5e-6 that keeps a bar of R * e_ref (R <= 8) meaningful."""
import pytest
import torch

import tile_walk as TW

CUS = 256      # an MI355X


@pytest.mark.parametrize("family", TW.FAMILIES)
def test_every_walk_visits_every_tile_once(family):
    """This pins the restatement, not the kernels: whoever changes a walk in csrc/ changes tile_walk.walk with it."""
    for n in range(1, 1301):
        w = TW.walk(family, n, CUS)
        assert len(w) == TW.grid_size(family, n, CUS)
        assert TW.visits_each_tile_once(w, n), (family, n)


@pytest.mark.parametrize("family,mutant", [("convblock", "band_end_off_by_one"), ("split-f16", "xcd_stride_is_grid"),
                                           ("convblock", "no_early_return")])
def test_the_coverage_check_fails_on_a_mutant(family, mutant):
    fails = [n for n in range(1, 1301) if not TW.visits_each_tile_once(TW.walk(family, n, CUS, mutant), n)]
    print(f"{family} {mutant}: {len(fails)} of 1300 tile counts fail, the first at {fails[:1]}")
    assert fails, (family, mutant)
    # ... and where it bites: the stride only with several tiles per workgroup in the XCD form, the missing return only
    # where a band is shorter than its XCD's workgroups
    if mutant == "xcd_stride_is_grid":
        assert min(fails) == CUS + 1 and all(n > CUS for n in fails)
    if mutant == "no_early_return":
        assert all(any(not x for x in TW.walk(family, n, CUS)) for n in fails)
        assert 259 in fails      # levels 2 and 3 of case A


def test_case_premises_at_256_cus():
    rows = []
    for case in TW.CASES:
        r, bad = TW.premises(case, CUS)
        rows += r
        assert not bad, bad
    print("\n" + TW.premises_table(rows))
    assert TW.case_a(CUS) == (259, 18, 34) and TW.case_b(CUS) == (12, 80, 112)
    assert TW.level_tiles("split-f16", *TW.case_a(CUS)) == [1554, 518, 259, 259]
    assert TW.level_tiles("split-f16", *TW.case_b(CUS)) == [420, 144, 48, 12]
    assert TW.chunks("A", "split-f16", CUS) == [(42 * k, 42) for k in range(6)] + [(252, 7)]
    assert TW.chunks("A", "direct", CUS) == [(28 * k, 28) for k in range(9)] + [(252, 7)]
    assert TW.chunks("B", "convblock", CUS) == [(0, 6), (6, 6)]
    # the output-channel split of the reference handles: MT = 3 at level 0 of the 42, MT = 1 elsewhere
    assert [TW.cout_split_applies(n, CUS) for n in TW.level_tiles("split-f16", 42, 18, 34)] == [False, True, True, True]
    assert all(TW.cout_split_applies(n, CUS) for n in TW.level_tiles("split-f16", 7, 18, 34))


@pytest.mark.parametrize("stem,profile,case", [(TW.UNETS[2][1], p, c) for p, c in TW.UNET_CASES]
                         + [(TW.UNETS[1][1], p, c) for p, c in TW.UNET_CASES] + [(TW.NEXTS[1][1], p, c) for p, c in TW.NEXT_CASES])
def test_reference_noise_of_the_forward_cases(stem, profile, case):
    _, _, _, o64, e_ref = TW.forward_reference(stem, profile, case, CUS)
    for what, w, e in zip(("out", "feat_out"), o64, e_ref):
        if w is None:
            continue
        assert torch.isfinite(w).all(), what
        print(f"{stem} {profile} case {case} {what}: max|f64| = {float(w.abs().max()):.3g}, e_ref = {e:.3g}")
        assert 0 < e <= 5e-6, (what, e)
