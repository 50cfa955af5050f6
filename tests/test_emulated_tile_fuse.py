"""tests/tile_fuse_cases.py on the CPU-emulated build of the kernel sources (tests/emu): the index math, the barriers' phases and the plan
of the fused statistics + embed + first inverse column step (k_fft_cols<COLS_STAT_EMBED>) against the two launches it replaces.  This
proves nothing about the gfx950 build -- tests/test_gpu_tile_fuse.py (-m gpu) runs the same checks there, with the natural plans of
larger covers and the workload-like shape added.

Every row is a 64- or 128-wide grid of 512 or 1024 rows, two images."""
import os
import subprocess

import pytest

import parity_cases as PC
import tile_fuse_cases as TF
from steganosaurus_amd import binding as B

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
BY = {r["name"]: r for r in TF.SMALL + TF.TILE_ROWS}


@pytest.fixture(scope="module")
def emu():
    subprocess.run(["make", "-C", EMU_DIR], check=True, stdout=subprocess.DEVNULL)
    return B.load(os.path.join(EMU_DIR, "libtfft_emu.so"))


@pytest.mark.parametrize("r", TF.SMALL, ids=TF.ids(TF.SMALL))
def test_fused_step_equals_the_pair_at_every_column_length(emu, orc, r):
    TF.check_plan_row(emu, orc, PC.HostBufs, r)


@pytest.mark.parametrize("r", TF.PAIR_ROWS[:1], ids=TF.ids(TF.PAIR_ROWS[:1]))      # (the 2048-wide (3,4) plan: on the GPU)
def test_16_point_plans_keep_the_pair_whatever_the_knob(emu, orc, r):
    TF.check_pair_row(emu, orc, PC.HostBufs, r)


@pytest.mark.parametrize("kind", TF.TILE_LISTS)
@pytest.mark.parametrize("r", TF.TILE_ROWS, ids=TF.ids(TF.TILE_ROWS))
def test_tile_contents(emu, orc, r, kind):
    TF.check_tile_contents(emu, orc, PC.HostBufs, r, kind)


@pytest.mark.parametrize("name", ["t_L32", "t_L256"])
def test_one_walk_per_image_with_jitter_and_a_stream_shorter_than_the_lists(emu, orc, name):
    TF.check_walks_jitter(emu, orc, PC.HostBufs, BY[name])


@pytest.mark.parametrize("name", ["s_L32", "s_L256"])
def test_bracket_miss_takes_the_gated_tail_from_tmp(emu, orc, name):
    TF.check_bracket_miss(emu, PC.HostBufs, orc, BY[name])


def test_adaptive_fit_and_exact_capacities_keep_the_pair(emu, orc):
    TF.check_fallbacks(emu, orc, PC.HostBufs, BY["t_L32"])


def test_profiler_times_the_fused_launch_as_cols_fwd_b(emu, orc):
    TF.check_profiler(emu, orc, PC.HostBufs, BY["s_L32"])
