"""CPU-emulated run (tests/emu) of the batched stream pipelines with one walk per image (tfft_*_stream_batch_walks[_dev]) and of
tfft_lowfreq_mag_batch_dev: the shared-list call's bytes for n copies of one walk, the fp64 reference image by image for distinct keys.
Not the product path (see test_emulated.py); tests/test_gpu_walks_batch.py is the gate on the MI355X."""
import os
import subprocess

import pytest

import walks_cases as WC
from parity_cases import HostBufs
from steganosaurus_amd import binding as B

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def emu():
    subprocess.run(["make", "-C", EMU_DIR], check=True, stdout=subprocess.DEVNULL)
    return B.load(os.path.join(EMU_DIR, "libtfft_emu.so"))


def test_same_lists_give_the_shared_list_bytes_two_chunks(emu, orc):
    WC.check_same_lists(emu, orc, HostBufs, 128, 128, nimg=3, slots=2, secret=8, jitter=0.05, adaptive=True)


def test_same_lists_give_the_shared_list_bytes_chunk_of_nine(emu, orc):
    # >= 8 images per chunk: the default tile-resident read and the two-stream split (each half builds its own buckets)
    WC.check_same_lists(emu, orc, HostBufs, 128, 128, nimg=9, slots=9, secret=8, jitter=0.05, adaptive=False, center=True,
                        envs=({}, {"TFFT_STREAMS": "2"}, {"TFFT_TILE_READ": "0"}, {"TFFT_STATS_TILE": "2"}), host=False)


def test_same_lists_without_jitter_chunk_of_eight(emu, orc):
    # Eight images in one chunk take the tile-resident read by default; without jitter that is the per-image read with no phase options
    # (k_fft_cols<.., COLS_READ, PH = false, PI = true>), which no other case here launches.  128 x 128: the direct column plan
    WC.check_same_lists(emu, orc, HostBufs, 128, 128, nimg=8, slots=8, secret=8, jitter=0.0, adaptive=False, envs=({},), host=False)


@pytest.mark.parametrize("jitter,adaptive", [(0.0, False), (0.05, False), (0.0, True), (0.05, True)])
def test_distinct_keys_two_step_columns(emu, orc, jitter, adaptive):
    # PH = 512: the two-step column plan, buckets per (image, plane, row group, column tile)
    WC.check_distinct_keys(emu, orc, HostBufs, 128, 512, nimg=3, slots=2, secret=8, jitter=jitter, adaptive=adaptive,
                           envs=({}, {"TFFT_STATS_TILE": "2"}, {"TFFT_TILE_READ": "3"}))


def test_distinct_keys_padded_cover(emu, orc):
    # 100 x 300 pads to 128 x 512: the raw bits of the reference's stego, no round trip (the crop loses the stream in the reference too)
    WC.check_distinct_keys(emu, orc, HostBufs, 100, 300, nimg=2, slots=2, secret=8, jitter=0.05, adaptive=True)


def test_distinct_keys_direct_columns(emu, orc):
    WC.check_distinct_keys(emu, orc, HostBufs, 128, 128, nimg=4, slots=4, secret=8, jitter=0.05, adaptive=True, center=True,
                           envs=({}, {"TFFT_EMBED_DELTA": "0"}))


def test_errors(emu, orc):
    WC.check_errors(emu, orc, HostBufs)


def test_lowfreq_batch_is_the_single_image_call(emu, golden_dir):
    import ctypes as C
    host = C.CDLL(os.path.join(ROOT, "steganosaurus_amd", "libtfhost.so"))
    WC.check_lowfreq_batch(emu, host, HostBufs, golden_dir, max_pixels=300 * 300)
