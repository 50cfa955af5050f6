"""tests/tile_fuse_cases.py on the MI355X: the fused statistics + embed + first inverse column step (k_fft_cols<COLS_STAT_EMBED>) against
the two launches it replaces -- waves, LDS phases and register budgets are what the emulated twin (tests/test_emulated_tile_fuse.py)
cannot show.  Adds the natural column plans at their smallest covers and one workload-like launch that fuses by the default rule."""
import pytest

import parity_cases as PC
import phase_cases as PH
import tile_fuse_cases as TF
from steganosaurus_amd import binding as B

pytestmark = pytest.mark.gpu
BY = {r["name"]: r for r in TF.SMALL + TF.TILE_ROWS + TF.NATURAL + TF.PAIR_ROWS}


@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a real MI355X"
    torch.zeros(1, device="cuda")           # torch's HIP runtime first (see test_gpu_parity.py)
    return B.load()


@pytest.mark.parametrize("r", TF.SMALL + TF.NATURAL, ids=TF.ids(TF.SMALL + TF.NATURAL))
def test_fused_step_equals_the_pair_at_every_column_plan(lib, orc, r):
    TF.check_plan_row(lib, orc, PC.TorchBufs, r)


def test_1080p_fuses_by_the_default_rule(lib, orc):
    """4 x 1920x1080, 20 000 bins, jitter, no knob set: 2^24 bins per launch, the default plan is the fused one.  PH.check_phase_batch holds the
    default to the fp64 reference and the pair (knob at 0) to the default's bytes and usable_out"""
    TF.assert_takes(lib, orc, PC.TorchBufs, {}, 1920, 1080, True, slots=4)
    TF.assert_takes(lib, orc, PC.TorchBufs, {"TFFT_EMBED_TILE_FUSE": "0"}, 1920, 1080, False, slots=4)
    TF.assert_takes(lib, orc, PC.TorchBufs, {}, 1920, 1080, False, slots=2)      # a launch of two: below the size rule
    PH.check_phase_batch(lib, orc, PC.TorchBufs, 1920, 1080, 20000, nimg=4, slots=4, jitter=0.05, adaptive=False, n_oracle=1,
                         envs=({}, {"TFFT_EMBED_TILE_FUSE": "0"}), tile_modes=("3",))


@pytest.mark.parametrize("r", TF.PAIR_ROWS, ids=TF.ids(TF.PAIR_ROWS))
def test_16_point_plans_keep_the_pair_whatever_the_knob(lib, orc, r):
    TF.check_pair_row(lib, orc, PC.TorchBufs, r)


@pytest.mark.parametrize("kind", TF.TILE_LISTS)
@pytest.mark.parametrize("r", TF.TILE_ROWS, ids=TF.ids(TF.TILE_ROWS))
def test_tile_contents(lib, orc, r, kind):
    TF.check_tile_contents(lib, orc, PC.TorchBufs, r, kind)


@pytest.mark.parametrize("name", ["t_L32", "t_L256", "f2k_8"])
def test_one_walk_per_image_with_jitter_and_a_stream_shorter_than_the_lists(lib, orc, name):
    TF.check_walks_jitter(lib, orc, PC.TorchBufs, BY[name])


@pytest.mark.parametrize("name", ["s_L32", "s_L256", "f2k_8"])
def test_bracket_miss_takes_the_gated_tail_from_tmp(lib, orc, name):
    TF.check_bracket_miss(lib, PC.TorchBufs, orc, BY[name])


def test_adaptive_fit_and_exact_capacities_keep_the_pair(lib, orc):
    TF.check_fallbacks(lib, orc, PC.TorchBufs, BY["t_L32"])


def test_profiler_times_the_fused_launch_as_cols_fwd_b(lib, orc):
    TF.check_profiler(lib, orc, PC.TorchBufs, BY["s_L32"])
