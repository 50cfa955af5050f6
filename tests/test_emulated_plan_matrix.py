"""tests/plan_matrix_cases.py on the CPU-emulated build of the kernel sources (tests/emu): the index math of every column plan's
smallest cover.  This proves nothing about the gfx950 build -- tests/test_gpu_plan_matrix.py (-m gpu) runs the same table there.

Checks that stay GPU-only here (the `gpu_only` field of the table), with the time one run took on the emulator -- eight cores, four
checks at a time; what is kept ran in about 50 s or less, as the slowest cases of tests/test_emulated.py do:
    ts_5_6   (40x1100)    forward 53 s, delta 165 s, stats > 355 s
    ts_6_7   (40x5000)    forward 141 s, delta and walks stopped after 240 s; stats not run (four times the rows of ts_5_6)
    ts_7_7   (24x9000)    forward stopped after 240 s; delta and stats not run (more work than forward)
    f2k_4    (1030x70)    stats 92 s              f4k_4 (2050x70)   stats 151 s
    f2k_6x2  (1030x300)   delta not run: f2k_6, the same cover with two images instead of three, took 67 s
    f2k_7, f2k_7x2 (1030x600)   forward 61 s; delta not run (twice the rows of f2k_6)
    f2k_9, f2k_9x2 (1030x2100)  not run (eight times the rows of f2k_6)
    f4k_5    (2050x130)   delta 98 s
    f4k_6, f4k_7 (2050x300, 2050x600)   not run (two and four times the rows of f4k_5, whose forward took 25 s)
The rows at PW = 16384 stay: w_16k_L2 forward 3 s, delta 6 s; w_16k_L6 forward 22 s, delta 45 s, stats 18 s, limits 30 s.  The
tile-resident read runs at every row (the slowest, f4k_7, 38 s), and so do the plan and coverage assertions, which are host code.
No row was shrunk to fit: a smaller size reaches another plan."""
import os
import subprocess

import pytest

import parity_cases as PC
import plan_matrix_cases as PM
from steganosaurus_amd import binding as B

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")


@pytest.fixture(scope="module")
def emu():
    subprocess.run(["make", "-C", EMU_DIR], check=True, stdout=subprocess.DEVNULL)
    return B.load(os.path.join(EMU_DIR, "libtfft_emu.so"))


@pytest.fixture(scope="module")
def orc(orc):
    return PM.SharedOracle(orc)      # one fp64 reference per input, shared by the rows that ask for it again


def ids(rows):
    return [r["name"] for r in rows]


# the plan and the coverage conditions are host code: every row, the GPU-only ones included
@pytest.mark.parametrize("r", PM.ROWS, ids=ids(PM.ROWS))
def test_row_reaches_its_plan_and_its_lists_cover_it(emu, orc, r):
    PM.check_coverage(emu, orc, r)


@pytest.mark.parametrize("r", PM.forward_rows(emulated_only=True), ids=ids(PM.forward_rows(emulated_only=True)))
def test_forward_and_identity(emu, orc, r):
    PM.check_forward(emu, orc, r)


@pytest.mark.parametrize("r", PM.rows_of(check="delta", emulated_only=True), ids=ids(PM.rows_of(check="delta", emulated_only=True)))
def test_delta_embedding(emu, orc, r):
    PM.check_delta(emu, orc, PC.HostBufs, r)


@pytest.mark.parametrize("r", PM.rows_of(check="tile_read", emulated_only=True), ids=ids(PM.rows_of(check="tile_read", emulated_only=True)))
def test_tile_resident_read(emu, orc, r):
    PM.check_row_tile_read(emu, orc, PC.HostBufs, r)


@pytest.mark.parametrize("r", PM.rows_of("walks", check="walks", emulated_only=True), ids=ids(PM.rows_of("walks", check="walks", emulated_only=True)))
def test_walks_with_jitter_and_adaptive_alpha(emu, orc, r):
    PM.check_walks(emu, orc, PC.HostBufs, r)


@pytest.mark.parametrize("r", PM.rows_of("stats", check="stats", emulated_only=True), ids=ids(PM.rows_of("stats", check="stats", emulated_only=True)))
def test_histograms_and_batched_capacities(emu, r):
    PM.check_stats(emu, PC.HostBufs, r)


@pytest.mark.parametrize("r", PM.rows_of("limits", check="limits", emulated_only=True), ids=ids(PM.rows_of("limits", check="limits", emulated_only=True)))
def test_limits_above_8192_columns(emu, orc, r):
    PM.check_limits(emu, orc, PC.HostBufs, r)
