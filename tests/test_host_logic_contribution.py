"""CPU, no device library: the host logic of contribution pruning - contribution.prune_mask, the unpacking of the kernel's rows, the combinations
GutTrainer(contribution_prune_at=...) refuses before it touches a device, and the arguments of tools/train_colmap.py and tools/prune_splat.py."""
import importlib.util
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _stats(max_w, sum_w):
    import lichtfeld_studio_amd  # noqa: F401
    from lichtfeld_studio_amd.contribution import ContributionStats
    return ContributionStats(torch.tensor(max_w, dtype=torch.float32), torch.tensor(sum_w, dtype=torch.float64), torch.ones(len(max_w), dtype=torch.int64), 1)


def test_prune_mask_threshold_mode():
    from lichtfeld_studio_amd.contribution import RADSPLAT_THRESHOLD, prune_mask
    st = _stats([0.0, 0.00999, 0.01, 0.5, 0.999], [0, 1, 2, 3, 4])
    assert RADSPLAT_THRESHOLD == 0.01
    assert prune_mask(st, threshold=0.01).tolist() == [True, True, False, False, False]      # strictly below: float32(0.01) itself stays
    assert prune_mask(st, threshold=1e-30).tolist() == [True, False, False, False, False]     # threshold -> 0+: the never-blended rows only
    assert prune_mask(st, threshold=0.01).dtype == torch.bool


def test_prune_mask_keep_mode_marks_exactly_n_minus_k_lowest_index_first():
    from lichtfeld_studio_amd.contribution import prune_mask
    st = _stats([0.1] * 8, [3.0, 0.0, 1.0, 0.0, 1.0, 7.0, 0.0, 1.0])
    assert prune_mask(st, keep=8).tolist() == [False] * 8 and prune_mask(st, keep=100).tolist() == [False] * 8
    assert prune_mask(st, keep=0).tolist() == [True] * 8
    # three zeros (indices 1, 3, 6), three ones (2, 4, 7): the ties go by index
    assert prune_mask(st, keep=6).tolist() == [False, True, False, True, False, False, False, False]
    assert prune_mask(st, keep=4).tolist() == [False, True, True, True, False, False, True, False]
    assert prune_mask(st, keep=3).tolist() == [False, True, True, True, True, False, True, False]
    for k in range(9):
        assert int(prune_mask(st, keep=k).sum()) == 8 - k
    with pytest.raises(ValueError):
        prune_mask(st, keep=-1)


def test_prune_mask_takes_exactly_one_rule():
    from lichtfeld_studio_amd.contribution import prune_mask
    st = _stats([0.1, 0.2], [1.0, 2.0])
    with pytest.raises(ValueError, match="exactly one"):
        prune_mask(st)
    with pytest.raises(ValueError, match="exactly one"):
        prune_mask(st, threshold=0.01, keep=1)


def test_rows_unpack_to_maximum_count_and_fixed_point_sum():
    """the layout of include/lfs_gsplat.h: bits of max w | uint32 count | 64-bit sum with 24 fraction bits, little endian - counts above 2^31 and sums above 2^32 included"""
    import numpy as np
    from lichtfeld_studio_amd.contribution import FIX_BITS, fold_interval, unpack_stats
    rows = np.zeros((3, 4), np.uint32)
    rows[0] = [np.float32(0.75).view(np.uint32), 5, 3 << 22, 0]                # sum 0.75
    rows[1] = [np.float32(0.999).view(np.uint32), 0xFFFFFFF0, 0x80000000, 7]    # count just below 2^32, sum (7 * 2^32 + 2^31) / 2^24
    m, c, s = unpack_stats(torch.from_numpy(rows.view(np.int32)))
    assert m.tolist() == [0.75, float(np.float32(0.999)), 0.0]
    assert c.tolist() == [5, 0xFFFFFFF0, 0] and c.dtype == torch.int64
    assert s.tolist() == [3 << 22, 7 * 2 ** 32 + 2 ** 31, 0] and s.dtype == torch.int64
    assert float(s[0]) * 2.0 ** -FIX_BITS == 0.75
    assert fold_interval(1920, 1080) == 2071 and fold_interval(64, 48) == (2 ** 32 - 1) // 3072 and fold_interval(1 << 20, 1 << 20) == 1
    assert fold_interval(1920, 1080) * 1920 * 1080 < 2 ** 32


def test_constructor_refuses_the_combinations_without_touching_a_device():
    import lichtfeld_studio_amd  # noqa: F401
    from lichtfeld_studio_amd import scenes
    from lichtfeld_studio_amd.trainer import GutTrainer
    sc = scenes.syn_a(n=16, sh_degree=1)
    base = dict(iterations=100, rasterizer="fastgs", contribution_prune_at=(20,))
    for bad, word in [(dict(rasterizer="gut"), "3DGUT"), (dict(world=2), "one rank"), (dict(rasterizer="gut", sh_sharded=True), "3DGUT"), (dict(sh_sharded=True), "sh_sharded"),
                      (dict(strategy="mcmc"), "mcmc"), (dict(one_call=True), "one_call"), (dict(contribution_prune_at=(0,)), r"outside 1\.\.100"),
                      (dict(contribution_prune_at=(5, 101)), r"\[101\]"), (dict(contribution_threshold=0.0), r"\(0, 1\)"), (dict(contribution_threshold=1.0), r"\(0, 1\)"),
                      (dict(contribution_threshold=-0.5), r"\(0, 1\)")]:
        with pytest.raises(ValueError, match=word):
            GutTrainer(sc, torch.device("cpu"), **{**base, **bad})


def _tool(name):
    spec = importlib.util.spec_from_file_location(name + "_tool", os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_train_colmap_contribution_arguments():
    tool = _tool("train_colmap")
    ap = tool.build_parser()
    a = ap.parse_args(["-d", "x"])
    assert a.contribution_prune_at == [] and a.contribution_threshold == 0.01
    tool.check_args(a)
    a = ap.parse_args(["-d", "x", "-i", "7000", "--contribution-prune-at", "3000", "6000", "--contribution-threshold", "0.05"])
    assert a.contribution_prune_at == [3000, 6000] and a.contribution_threshold == 0.05
    tool.check_args(a)
    with pytest.raises(SystemExit, match="not wired into the 3DGUT route"):
        tool.check_args(ap.parse_args(["-d", "x", "--contribution-prune-at", "100", "--gut"]))
    with pytest.raises(SystemExit, match="mcmc"):
        tool.check_args(ap.parse_args(["-d", "x", "--contribution-prune-at", "100", "--strategy", "mcmc"]))
    with pytest.raises(SystemExit, match=r"outside 1\.\.500"):
        tool.check_args(ap.parse_args(["-d", "x", "-i", "500", "--contribution-prune-at", "100", "501"]))
    with pytest.raises(SystemExit, match="outside"):
        tool.check_args(ap.parse_args(["-d", "x", "--contribution-prune-at", "0"]))
    for bad in ("0", "1", "-0.1"):
        with pytest.raises(SystemExit, match=r"\(0, 1\)"):
            tool.check_args(ap.parse_args(["-d", "x", "--contribution-prune-at", "100", "--contribution-threshold", bad]))
    tool.check_args(ap.parse_args(["-d", "x", "--gut", "--contribution-threshold", "5"]))     # (without prune iterations the threshold is not looked at: nothing is on)
    with pytest.raises(SystemExit, match="--antialiasing is not wired into the 3DGUT route"):
        tool.check_args(ap.parse_args(["-d", "x", "--antialiasing", "--gut"]))               # (the earlier refusals are where they were)


def test_prune_splat_arguments():
    tool = _tool("prune_splat")
    ap = tool.build_parser()
    a = ap.parse_args(["-d", "x", "--ply", "in.ply", "--out", "o", "--threshold", "0.01"])
    assert (a.threshold, a.keep, a.images, a.save_sog) == (0.01, None, "images", False)
    tool.check_args(a)
    a = ap.parse_args(["-d", "x", "--ply", "in.ply", "--out", "o.ply", "--keep", "1000", "--images", "images_4", "--save-sog"])
    assert (a.threshold, a.keep, a.images, a.save_sog) == (None, 1000, "images_4", True)
    tool.check_args(a)
    with pytest.raises(SystemExit, match="exactly one"):
        tool.check_args(ap.parse_args(["-d", "x", "--ply", "in.ply", "--out", "o"]))
    with pytest.raises(SystemExit, match="exactly one"):
        tool.check_args(ap.parse_args(["-d", "x", "--ply", "in.ply", "--out", "o", "--threshold", "0.01", "--keep", "5"]))
    for bad in ("0", "1.0"):
        with pytest.raises(SystemExit, match=r"\(0, 1\)"):
            tool.check_args(ap.parse_args(["-d", "x", "--ply", "in.ply", "--out", "o", "--threshold", bad]))
    with pytest.raises(SystemExit, match="--keep"):
        tool.check_args(ap.parse_args(["-d", "x", "--ply", "in.ply", "--out", "o", "--keep", "0"]))
    with pytest.raises(SystemExit, match=".ply"):
        tool.check_args(ap.parse_args(["-d", "x", "--ply", "in.sog", "--out", "o", "--keep", "5"]))
    with pytest.raises(SystemExit):
        ap.parse_args(["--ply", "in.ply", "--out", "o", "--keep", "5"])                        # -d is required
