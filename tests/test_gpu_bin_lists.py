"""tests/bin_list_cases.py on the MI355X: the bucketed column kernels (COLS_READ / COLS_EMBED / COLS_EMIT / COLS_STAT, k_bucket_*,
k_bins_last_row) on whole-plane, hand-built bin lists against a numpy fp64 reference.  The emulated twin is
tests/test_emulated_bin_lists.py."""
import pytest

import bin_list_cases as BL
import parity_cases as PC
from steganosaurus_amd import binding as B

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a real MI355X"
    torch.zeros(1, device="cuda")           # torch's HIP runtime first (see test_gpu_parity.py)
    return B.load()


def ids(rows):
    return [r["name"] for r in rows]


@pytest.mark.parametrize("r", BL.ROWS, ids=ids(BL.ROWS))
def test_row_reaches_its_plan_and_its_lists_are_valid(lib, orc, r):
    BL.check_builders(lib, orc, r)


@pytest.mark.parametrize("c", BL.shared_cases(), ids=[BL.case_id(c) for c in BL.shared_cases()])
def test_shared_list_embed_and_extract(lib, orc, c):
    BL.check_shared(lib, orc, PC.TorchBufs, *c)


@pytest.mark.parametrize("c", BL.usable_cases(), ids=[BL.usable_id(c) for c in BL.usable_cases()])
def test_usable_out_does_not_depend_on_the_list(lib, c):
    BL.check_usable(lib, PC.TorchBufs, *c)


@pytest.mark.parametrize("r", BL.rows(walks=True), ids=ids(BL.rows(walks=True)))
def test_one_list_per_image_with_jitter_and_adaptive_alpha(lib, orc, r):
    BL.check_walks(lib, orc, PC.TorchBufs, r)


@pytest.mark.parametrize("r", BL.rows(host=True), ids=ids(BL.rows(host=True)))
def test_host_forms_return_the_bytes_of_the_dev_calls(lib, r):
    BL.check_host_form(lib, PC.TorchBufs, r)
