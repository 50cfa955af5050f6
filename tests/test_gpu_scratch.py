"""The checks of tests/scratch_cases.py on the MI355X: the host forms of the analysis, robustness and SPAM calls interleaved on one context
(they share one scratch), the scratch replaced under a _dev call that is still running, and calls that are no multiple of n_slots."""
import pytest

import scratch_cases as XC
from parity_cases import TorchBufs
from steganosaurus_amd import binding as B

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    # torch's HIP runtime first: initialised after the library's in the same process it finds no device
    import torch
    assert torch.cuda.is_available()
    torch.zeros(1, device="cuda")


@pytest.fixture(scope="module")
def lib():
    return B.load()


def test_interleaved_host_forms_on_one_context(lib):
    XC.check_interleaved(lib, TorchBufs)


def test_growth_under_an_unfinished_call(lib):
    XC.check_growth_under_unfinished_call(lib, TorchBufs)


@pytest.mark.parametrize("n,slots", [(1, 2), (3, 1)])
def test_calls_that_are_no_multiple_of_the_slots(lib, orc, n, slots):
    XC.check_partial_chunks(lib, orc, TorchBufs, n, slots)
