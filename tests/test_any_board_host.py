"""Host-side checks of the any-board tower / projector domain (no GPU): pmx_actor_supported and pmx_actor_sizes are plain host
functions of the library, and the tools' new board options parse and build their layouts without touching a device."""
import ctypes as C
import importlib.util
import os

import pytest

import _tower_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sizes(lib, H, W, B):
    sv, sc, si = C.c_int64(-1), C.c_int64(-1), C.c_int64(-1)
    rc = lib.pmx_actor_sizes(H, W, B, C.byref(sv), C.byref(sc), C.byref(si))
    return rc, sv.value, sc.value, si.value


def test_supported_is_exactly_the_640_cell_domain():
    """1 on every board with W in 8..32, H in 3..32 and H * W <= 640 (tile counts 2 .. 44), 0 on larger boards and on sides out
    of range; pmx_actor_sizes follows it."""
    import pmx
    lib = pmx._lib.load()
    seen = set()
    for H in range(-1, 36):
        for W in range(-1, 36):
            want = 1 if R.in_domain(H, W) else 0
            assert lib.pmx_actor_supported(H, W) == want, (H, W)
            rc = _sizes(lib, H, W, 4)[0]
            assert (rc == 0) == bool(want), (H, W, rc)
            if want:
                seen.add(R.tiles(H, W))
                assert R.bucket(R.tiles(H, W)) > 0
    assert min(seen) == 2 and max(seen) == 44
    assert lib.pmx_actor_supported(26, 25) == 0 and lib.pmx_actor_supported(32, 32) == 0          # 650 and 1 024 cells


@pytest.mark.parametrize("board", [(3, 8), (12, 14), (16, 14), (9, 16), (7, 20), (13, 18), (20, 20), (16, 27), (16, 32), (18, 30), (17, 32),
                                   (32, 18), (20, 32), (32, 20)])
def test_sizes_are_monotone_and_cover_the_bucket(board):
    """Monotone in B, and at least what the kernels of the board's BUCKET address: 16 P-layout dumps of the bucket's tiles and the
    GroupNorm statistics per sample; per sample 8 layers of dH operand fragments (bucket key-pair blocks), then the skip slots
    (<= 2 048), 1 024 rows of bias / affine partial sums and <= 128 rows of weight partial sums.  Never less than the
    board's own tile count needs."""
    import pmx
    lib = pmx._lib.load()
    H, W = board
    nb = R.bucket(R.tiles(H, W))
    assert nb >= R.tiles(H, W)
    prev = (0, 0, 0)
    for B in (0, 1, 2, 5, 64, 65, 1300, 8192):
        rc, sv, sc, si = _sizes(lib, H, W, B)
        assert rc == 0
        dump = nb * 1024
        assert sv >= B * (16 * dump + 8 * 4 * 2 * 4)
        assert si >= 2048 * dump
        assert sc >= B * 8 * ((nb + 1) // 2) * 2048 + 2048 * dump + 1024 * 768 * 4 + 128 * 8 * 36 * 256 * 4
        assert sv >= prev[0] and sc >= prev[1] and si >= prev[2]
        prev = (sv, sc, si)
    assert _sizes(lib, H, W, -1)[0] != 0


def _tool(name):
    spec = importlib.util.spec_from_file_location("pmx_tool_" + name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)                 # the tools run under `if __name__ == "__main__"` only
    return mod


@pytest.mark.parametrize("tool", ["train", "train_bench"])
def test_maze_size_option_builds_32x16_layouts(tool):
    mod = _tool(tool)
    args = mod.parser().parse_args(["--layout", "mazes", "--maze-size", "32x16", "--envs", "3"])
    assert args.maze_size == (32, 16)
    lays = mod.layouts(args)
    assert len(lays) == 3 and all((l.width, l.height) == (32, 16) and len(l.agent_positions) == 4 for l in lays)
    assert len({tuple(l.text) for l in lays}) == 3                                        # one distinct maze per env
    # the default is the 20 x 20 board of today, and a named layout stays a name
    d = mod.parser().parse_args(["--layout", "mazes", "--envs", "2"])
    assert d.maze_size == (20, 20)
    assert all((l.width, l.height) == (20, 20) for l in mod.layouts(d))
    assert mod.layouts(mod.parser().parse_args([])) == "smallCapture"
    for bad in ("31x16", "32", "40x16", "32x2", "axb"):
        with pytest.raises(SystemExit):
            mod.parser().parse_args(["--maze-size", bad])


def test_train_mazes_use_disjoint_seeds_per_rank():
    mod = _tool("train")
    args = mod.parser().parse_args(["--layout", "mazes", "--maze-size", "32x16", "--envs", "2"])
    a, b = mod.layouts(args, 0), mod.layouts(args, 1)
    assert len({tuple(l.text) for l in a + b}) == 4


def test_actor_bench_board_option():
    mod = _tool("actor_bench")
    args = mod.parser().parse_args(["--board", "16x32", "--batch", "512", "8192"])
    assert args.board == (16, 32) and args.batch == [512, 8192]
    assert mod.board_of(args) == (16, 32, "16x32")
    assert mod.board_of(mod.parser().parse_args(["--layout", "tinyCapture"])) == (7, 20, "tinyCapture")
    with pytest.raises(SystemExit):
        mod.parser().parse_args(["--board", "16"])
