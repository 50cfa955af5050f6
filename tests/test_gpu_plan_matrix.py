"""tests/plan_matrix_cases.py on the MI355X: the batched pipelines (bucket modes of k_fft_cols) at the smallest cover of every column
plan, against the fp64 oracle.  The emulated twin is tests/test_emulated_plan_matrix.py."""
import pytest

import parity_cases as PC
import plan_matrix_cases as PM
from steganosaurus_amd import binding as B

pytestmark = pytest.mark.gpu
IDS = [r["name"] for r in PM.ROWS]


@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a real MI355X"
    torch.zeros(1, device="cuda")           # torch's HIP runtime first (see test_gpu_parity.py)
    return B.load()


@pytest.fixture(scope="module")
def orc(orc):
    return PM.SharedOracle(orc)      # one fp64 reference per input, shared by the rows that ask for it again


def ids(rows):
    return [r["name"] for r in rows]


@pytest.mark.parametrize("r", PM.ROWS, ids=IDS)
def test_row_reaches_its_plan_and_its_lists_cover_it(lib, orc, r):
    PM.check_coverage(lib, orc, r)


@pytest.mark.parametrize("r", PM.forward_rows(), ids=ids(PM.forward_rows()))
def test_forward_and_identity(lib, orc, r):
    PM.check_forward(lib, orc, r)


@pytest.mark.parametrize("r", PM.ROWS, ids=IDS)
def test_delta_embedding(lib, orc, r):
    PM.check_delta(lib, orc, PC.TorchBufs, r)


@pytest.mark.parametrize("r", PM.ROWS, ids=IDS)
def test_tile_resident_read(lib, orc, r):
    PM.check_row_tile_read(lib, orc, PC.TorchBufs, r)


@pytest.mark.parametrize("r", PM.rows_of("walks"), ids=ids(PM.rows_of("walks")))
def test_walks_with_jitter_and_adaptive_alpha(lib, orc, r):
    PM.check_walks(lib, orc, PC.TorchBufs, r)


@pytest.mark.parametrize("r", PM.rows_of("stats"), ids=ids(PM.rows_of("stats")))
def test_histograms_and_batched_capacities(lib, r):
    PM.check_stats(lib, PC.TorchBufs, r)


@pytest.mark.parametrize("r", PM.rows_of("limits"), ids=ids(PM.rows_of("limits")))
def test_limits_above_8192_columns(lib, orc, r):
    PM.check_limits(lib, orc, PC.TorchBufs, r)
