"""tests/bin_list_cases.py on the CPU-emulated build of the kernel sources (tests/emu): the index math of the bucketed column kernels
on whole-plane, hand-built bin lists.  This proves nothing about the gfx950 build -- tests/test_gpu_bin_lists.py (-m gpu) runs the
same table there, and the rows the emulator cannot afford (ROWS with emu=False) only there.

Time of one run on the emulator (eight cores, this module alone: 76 tests, 11 minutes in all); every case stays at about 50 s:
    plans, lists and bucket figures (host code, all ten rows)     <= 1.2 s each
    shared list, embed + extract    p2_direct, d_L4, n_M8 <= 0.9 s per list; p2_two_step 1.0 - 1.8 s; ts_pad 2.0 - 2.8 s;
                                    p2_f2k_4: dense x3 20 - 22 s, tiles_alternate 15 s, the other tiles lists and frame 8 - 9 s
    usable_out, per statistics variant (default / TFFT_STATS_TILE=2 / =0; every embed of a row's lists runs the statistics stage)
                                    d_L4 2 - 3 s, n_M8 6 - 7 s, p2_direct 11 / 14 / 14 s, ts_pad 37 / 20 / 45 s,
                                    p2_two_step 44 / 21 / 48 s, p2_f2k_4 31 / 51 / 37 s
    one list per image              p2_direct 5 s, p2_two_step 28 s, ts_pad 28 s, p2_f2k_4 36 s
    host forms                      p2_direct 2.5 s
GPU only, not run here: ts_5_6 (40x1100: PM's delta check of the same cover took 165 s), f2k_6x2 and f4k_4 (four and two times the
grid of p2_f2k_4, three images per call), f2k_9 (32 times that grid)."""
import os
import subprocess

import pytest

import bin_list_cases as BL
import parity_cases as PC
from steganosaurus_amd import binding as B

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")


@pytest.fixture(scope="module")
def emu():
    subprocess.run(["make", "-C", EMU_DIR], check=True, stdout=subprocess.DEVNULL)
    return B.load(os.path.join(EMU_DIR, "libtfft_emu.so"))


def ids(rows):
    return [r["name"] for r in rows]


# the plans, the lists and the bucket figures are host code: every row, the GPU-only ones included
@pytest.mark.parametrize("r", BL.ROWS, ids=ids(BL.ROWS))
def test_row_reaches_its_plan_and_its_lists_are_valid(emu, orc, r):
    BL.check_builders(emu, orc, r)


@pytest.mark.parametrize("c", BL.shared_cases(emulated=True), ids=[BL.case_id(c) for c in BL.shared_cases(emulated=True)])
def test_shared_list_embed_and_extract(emu, orc, c):
    BL.check_shared(emu, orc, PC.HostBufs, *c)


@pytest.mark.parametrize("c", BL.usable_cases(emulated=True), ids=[BL.usable_id(c) for c in BL.usable_cases(emulated=True)])
def test_usable_out_does_not_depend_on_the_list(emu, c):
    BL.check_usable(emu, PC.HostBufs, *c)


@pytest.mark.parametrize("r", BL.rows(emulated=True, walks=True), ids=ids(BL.rows(emulated=True, walks=True)))
def test_one_list_per_image_with_jitter_and_adaptive_alpha(emu, orc, r):
    BL.check_walks(emu, orc, PC.HostBufs, r)


@pytest.mark.parametrize("r", BL.rows(emulated=True, host=True), ids=ids(BL.rows(emulated=True, host=True)))
def test_host_forms_return_the_bytes_of_the_dev_calls(emu, r):
    BL.check_host_form(emu, PC.HostBufs, r)
