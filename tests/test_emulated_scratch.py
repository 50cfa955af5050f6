"""CPU-emulated run (tests/emu) of the checks of tests/scratch_cases.py: the host forms of the analysis, robustness and SPAM calls
interleaved on one context (they share one scratch), the scratch replaced under a call that has not finished (trivially ordered here: the
emulated runtime runs every call to its end), and calls that are no multiple of n_slots.  Not the product path (see test_emulated.py);
tests/test_gpu_scratch.py is the gate on the MI355X."""
import os
import subprocess

import pytest

import scratch_cases as XC
from parity_cases import HostBufs
from steganosaurus_amd import binding as B

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")


@pytest.fixture(scope="module")
def emu():
    subprocess.run(["make", "-C", EMU_DIR], check=True, stdout=subprocess.DEVNULL)
    return B.load(os.path.join(EMU_DIR, "libtfft_emu.so"))


def test_interleaved_host_forms_on_one_context(emu):
    XC.check_interleaved(emu, HostBufs)


def test_growth_under_an_unfinished_call(emu):
    XC.check_growth_under_unfinished_call(emu, HostBufs)


@pytest.mark.parametrize("n,slots", [(1, 2), (3, 1)])
def test_calls_that_are_no_multiple_of_the_slots(emu, orc, n, slots):
    XC.check_partial_chunks(emu, orc, HostBufs, n, slots)
