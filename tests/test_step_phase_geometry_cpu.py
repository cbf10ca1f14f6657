"""helpers.qde_geometry -- the restated launch geometry of the long item-side backward kernel (csrc/qde_pieces.h) -- held
to rows worked out by hand and to the C code itself.  The GPU tests assert the form and the cut they claim to exercise against this helper
(tests/test_gpu_step_phases.py), and the shape tables in the comments of tests/test_gpu_qhead_grad_rows.py and
tests/test_gpu_train.py are its rows at 256 CUs.

How a row is worked: groups of 256 items (128 for d = 256), stages of 64 states (32 for d = 256), W = G T stage-units
dealt to grid = min(W, CUs) blocks; block p starts at unit floor(p W / grid), inside a group iff that is no multiple of T.
With W <= CUs every block holds one unit, so the kernel cuts as soon as T > 1."""
import os

import pytest

from helpers import qde_geometry

# (B, N, d, n_cu) -> (form, G, T, W, grid, cut)
ROWS = [
    # the shapes of tests/test_gpu_step_phases.py
    ((128, 1000, 128, 256), ("qde2", 4, 2, 8, 8, True)),                  # starts 0..7: 1 % 2 != 0
    ((96, 1000, 128, 256), ("qde_kernel<128>", 4, 2, 8, 8, True)),        # 96 % 64 != 0: generic kernel, T = ceil(96 / 64)
    ((64, 1000, 256, 256), ("qde3", 8, 2, 16, 16, True)),                 # 128-item groups, 32-state stages
    ((128, 2000, 64, 256), ("qde_kernel<64>", 8, 2, 16, 16, True)),
    ((64, 5003, 128, 256), ("qde2", 20, 1, 20, 20, False)),               # T = 1: every unit is a whole group
    ((1024, 5003, 128, 256), ("qde2", 20, 16, 320, 256, True)),           # W > CUs: block 1 starts at 320 / 256 = 1
    # the rows of the comment tables that said "no"
    ((100, 1000, 128, 256), ("qde_kernel<128>", 4, 2, 8, 8, True)),
    ((128, 100, 128, 256), ("qde2", 1, 2, 2, 2, True)),                   # one group, two blocks: block 1 starts at stage 1
    # the other rows of the two tables
    ((1024, 20011, 128, 256), ("qde2", 79, 16, 1264, 256, True)),
    ((1000, 20011, 128, 256), ("qde_kernel<128>", 79, 16, 1264, 256, True)),
    ((512, 5003, 256, 256), ("qde3", 40, 16, 640, 256, True)),
    ((500, 5003, 256, 256), ("qde_kernel<256>", 40, 16, 640, 256, True)),
    ((1024, 20011, 64, 256), ("qde_kernel<64>", 79, 16, 1264, 256, True)),
    ((1, 3001, 128, 256), ("qde_kernel<128>", 12, 1, 12, 12, False)),
    ((1, 777, 256, 256), ("qde_kernel<256>", 7, 1, 7, 7, False)),
    ((256, 5003, 256, 256), ("qde3", 40, 8, 320, 256, True)),
    # the cut depends on the CU count: 8 units over 4 blocks start at 0, 2, 4, 6 (whole groups), over 3 at 0, 2, 5
    ((128, 1000, 128, 4), ("qde2", 4, 2, 8, 4, False)),
    ((128, 1000, 128, 3), ("qde2", 4, 2, 8, 3, True)),
    ((1024, 5003, 128, 64), ("qde2", 20, 16, 320, 64, True)),             # starts 5 p
    ((1024, 5003, 128, 20), ("qde2", 20, 16, 320, 20, False)),            # starts 16 p: one group per block
    # a CU count the library does not believe counts as 256
    ((1024, 5003, 128, 304), ("qde2", 20, 16, 320, 256, True)),
    ((1024, 5003, 128, 0), ("qde2", 20, 16, 320, 256, True)),
]


@pytest.mark.parametrize("args,want", ROWS, ids=[f"B{a[0]}-N{a[1]}-d{a[2]}-cu{a[3]}" for a, _ in ROWS])
def test_hand_worked_rows(args, want):
    assert qde_geometry(*args) == want


def test_helper_agrees_with_the_c_plan_on_every_row():
    """helpers.qde_geometry against csrc/qde_pieces.h itself -- qde_plan and QdePieces::any_cut, the code cql_qde_launch
    runs -- through the stand-alone host driver's `qde_plan` mode (tests/asan/host_driver.cpp; nothing is loaded into
    Python), over every shape and CU count of ROWS"""
    import subprocess
    from replay_cql_amd import build as B
    exe = B.build_asan()
    argv = [str(x) for args, _ in ROWS for x in args]
    r = subprocess.run([str(exe), "qde_plan"] + argv, capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0", HIP_VISIBLE_DEVICES=""))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == len(ROWS)
    for (args, _), line in zip(ROWS, lines):
        form, G, T, W, grid, cut = line.split()
        assert (form, int(G), int(T), int(W), int(grid), bool(int(cut))) == qde_geometry(*args), (args, line)


def test_small_shapes_cut_as_soon_as_there_are_two_stages():
    """W <= CUs: grid = W, block p starts at unit p, and p = 1 is inside group 0 whenever T > 1."""
    for d in (64, 128, 256):
        for B in (1, 32, 33, 64, 65, 96, 128, 200):
            for N in (1, 100, 129, 257, 1000):
                form, G, T, W, grid, cut = qde_geometry(B, N, d, 256)
                if W <= 256:
                    assert grid == W and cut == (T > 1), (B, N, d)
                assert form == ("qde2" if d == 128 and B % 64 == 0 else "qde3" if d == 256 and B % 32 == 0 else
                                f"qde_kernel<{d}>")


def test_cut_is_the_statement_about_block_starts():
    """the predicate, brute force: cut <=> some block but the first starts at a unit that is not the first of its group"""
    for B, N, d in ((128, 1000, 128), (1024, 5003, 128), (256, 5003, 256), (512, 20011, 64)):
        for n_cu in (1, 2, 3, 7, 16, 20, 64, 255, 256):
            _, G, T, W, grid, cut = qde_geometry(B, N, d, n_cu)
            starts = [p * W // grid for p in range(grid)]
            assert starts[0] == 0 and all(b > a for a, b in zip(starts, starts[1:]))
            assert cut == any(s % T for s in starts[1:]), (B, N, d, n_cu)
