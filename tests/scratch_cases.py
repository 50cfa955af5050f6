"""The analysis scratch shared by the analysis, robustness and SPAM calls, and the chunk loop of their host forms (DESIGN.md sections 12 to
14), written once and run twice: on the CPU-emulated build (tests/test_emulated_scratch.py) and on the MI355X (tests/test_gpu_scratch.py,
-m gpu).

Every call family lays its arrays out afresh in the one buffer, so what can go wrong is a call that reads what another family left there, a
buffer replaced under a call that has not finished, and a partial last chunk.  Nothing here restates a reference: the _dev forms are held
to theirs by the tests of their own families, and every result below is compared with == (bit for bit) against a _dev form on a fresh
context."""
import functools
from collections import namedtuple

import numpy as np

import analysis_cases as AC
import fit_cases as FC
import robust_cases as RC
import spam_cases as SC
from steganosaurus_amd import binding as B
from steganosaurus_amd.synth import cover_rgb

MAX, SLOTS, N = 128, 2, 5                        # 5 images in 2 slots: chunks of 2, 2 and 1
AWGN = ("awgn", 2.0, 7)
ROBUST_CHANNELS = [("none",), AWGN, ("jpeg", 75)]

# host(ctx, n) / dev(bufs, ctx): the call over the first n / over all `n` images of its input, as a tuple of arrays; axis: the image axis
Step = namedtuple("Step", "name n axis host dev")


def covers(w, h, seed, n=N):
    return np.stack([cover_rgb(w, h, seed + i) for i in range(n)])


def quality_dev(bufs, ctx, a, b, ssim=True):
    """issues the _dev form and returns the function that synchronises and fetches (sse[, ssim])"""
    n, h, w = a.shape[:3]
    ins = [bufs.put(a), bufs.put(b)]
    outs = [bufs.put(np.zeros((n, 3), np.uint64))] + ([bufs.put(np.zeros((n, 3), np.float64))] if ssim else [])
    ctx.quality_batch_dev(n, ins[0][1], ins[1][1], w, h, outs[0][1], outs[1][1] if ssim else None)

    def finish():
        ctx.sync()
        assert np.array_equal(np.asarray(bufs.get(ins[0][0])).reshape(a.shape), a), "an input was written"
        return tuple(np.asarray(bufs.get(o[0])).reshape(n, 3).copy() for o in outs)
    return finish


def steps(inp):
    """the sequence of test 1, in its order"""
    case = inp["case"]

    def robust_host(ctx, n):
        return (ctx.robustness_batch_host(case["stego"][:n], case["ubins"], case["hdr"][:n], case["pay"][:n], ROBUST_CHANNELS, alpha=case["alpha"],
                                          center=case["center"], first_image=5),)

    def spam(key, t):
        x = inp[key]
        return Step("%s t=%d" % (key, t), N, 0, lambda ctx, n: (ctx.spam_batch_host(x[:n], t=t),), lambda bufs, ctx: (SC.spam_dev(bufs, ctx, x, t),))

    def quality(key, ssim):
        a, b = inp[key]
        return Step(key, N, 0, lambda ctx, n: tuple(r for r in ctx.quality_batch_host(a[:n], b[:n], ssim=ssim) if r is not None),
                    lambda bufs, ctx: quality_dev(bufs, ctx, a, b, ssim)())

    return [spam("spam 48x40", 1),
            quality("quality 64x64", True),
            Step("awgn 101x37", N, 0, lambda ctx, n: (ctx.channel_batch_host(inp["awgn 101x37"][:n], AWGN, first_image=3),),
                 lambda bufs, ctx: (RC.run_channel(bufs, ctx, inp["awgn 101x37"], AWGN, first_image=3),)),
            Step("robustness 128x128", case["n"], 1, robust_host, lambda bufs, ctx: (RC.run_robust_dev(bufs, ctx, case, ROBUST_CHANNELS, first_image=5),)),
            Step("hist 64x64", N, 0, lambda ctx, n: (ctx.phase_hist_batch_host(inp["hist 64x64"][:n], nbins=4096),),
                 lambda bufs, ctx: (AC.hist_dev(None, bufs, ctx, inp["hist 64x64"], 4096),)),
            spam("spam 128x128", 4),
            quality("quality 48x40", False)]


def context(lib, inp, slots=SLOTS):
    ctx = B.Context(MAX, MAX, slots=slots, lib=lib)
    RC.configure(ctx, inp["case"]["idx"], inp["case"]["jit"], inp["case"]["phase"])
    return ctx


_LIBS = {}


@functools.lru_cache(maxsize=None)
def _references(lib_id, bufs):
    lib = _LIBS[lib_id]
    inp = {"spam 48x40": covers(48, 40, 200), "quality 64x64": (covers(64, 64, 210), AC.perturbed(covers(64, 64, 210), 1)),
           "awgn 101x37": covers(101, 37, 220), "case": RC.make_case(lib, bufs, 128, 128, 3, 16, True, False, center=True, extra_bins=0),
           "hist 64x64": covers(64, 64, 230), "spam 128x128": covers(128, 128, 240),
           "quality 48x40": (covers(48, 40, 250), AC.perturbed(covers(48, 40, 250), 2))}
    want = {}
    for st in steps(inp):
        ctx = context(lib, inp)
        try:
            want[st.name] = st.dev(bufs, ctx)
        finally:
            ctx.close()
    ctx = context(lib, inp)      # (what RC.check_channel_forms returns: the images counted from 0)
    try:
        want["awgn 101x37, first image 0"] = (RC.run_channel(bufs, ctx, inp["awgn 101x37"], AWGN),)
    finally:
        ctx.close()
    return inp, want


@functools.lru_cache(maxsize=None)
def _fit_reference(lib_id, bufs, orc):
    """five covers of 100 x 120 (padded to 128 x 128) with their own walks, and the _dev form's (stego, usable, iters, wrong) in 2 slots"""
    batch = FC.make_batch(orc, 100, 120, N, jitter=0.05, tag=b"scratch", lib=_LIBS[lib_id])
    return batch, FC.run_fit(_LIBS[lib_id], bufs, batch, SLOTS, False, False, max_iters=8)


def references(lib, bufs):
    """(inputs, the _dev form's result of every step on a context of its own): computed once per library, read only"""
    _LIBS[id(lib)] = lib
    return _references(id(lib), bufs)


def same(got, want, tag, n=None, axis=0):
    """got == the first n images of want, array by array, bit for bit"""
    assert len(got) == len(want), tag
    for g, w in zip(got, want):
        w = w if n is None else np.take(w, range(n), axis=axis)
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == np.ascontiguousarray(w).tobytes(), tag


def check_interleaved(lib, bufs):
    """test 1: the host forms of every family one after the other on one context, twice; the second round grows nothing"""
    inp, want = references(lib, bufs)
    ctx = context(lib, inp)
    try:
        sizes = []
        for rnd in range(2):
            for st in steps(inp):
                same(st.host(ctx, st.n), want[st.name], (rnd, st.name))
            sizes.append(ctx.device_bytes())
        print("tfft_device_bytes after the sequence:", sizes[0])
        assert sizes[1] == sizes[0], sizes
    finally:
        ctx.close()


def check_growth_under_unfinished_call(lib, bufs):
    """test 2: a _dev call whose partials lie in the scratch is still running when a host form replaces the scratch by a larger one"""
    inp, want = references(lib, bufs)
    a, b = inp["quality 64x64"]
    ctx = context(lib, inp)
    try:
        finish = quality_dev(bufs, ctx, a, b)
        before = ctx.device_bytes()
        counts = ctx.spam_batch_host(inp["spam 128x128"], t=4)
        assert ctx.device_bytes() > before, "the SPAM call did not have to grow the scratch"
        same(finish(), want["quality 64x64"], "quality under growth")
        same((counts,), want["spam 128x128 t=4"], "the growing call")
    finally:
        ctx.close()


def check_partial_chunks(lib, orc, bufs, n, slots):
    """test 3: n images in `slots` slots through every rebuilt host form == the first n of the 5-image results"""
    inp, want = references(lib, bufs)
    ctx = context(lib, inp, slots)
    try:
        for st in steps(inp):
            m = min(n, st.n)
            same(st.host(ctx, m), want[st.name], (n, slots, st.name), m, st.axis)
    finally:
        ctx.close()
    # the families' own chunk checks at these counts: host == _dev == the images one by one
    same((SC.check_batch_equals_singles(lib, bufs, inp["spam 128x128"][:n], slots, t=4),), want["spam 128x128 t=4"], "spam", n)
    same((AC.check_hist_chunks(lib, bufs, inp["hist 64x64"][:n], nbins=4096, slots=slots),), want["hist 64x64"], "hist", n)
    same((RC.check_channel_forms(lib, bufs, inp["awgn 101x37"][:n], AWGN, slots),), want["awgn 101x37, first image 0"], "channel", n)
    # the fitted embed: the host form of the first n == the _dev form of all five
    batch, whole = _fit_reference(id(lib), bufs, orc)
    part = dict(batch, **{k: batch[k][:n] for k in ("covers", "bins", "jit", "headers", "payloads")})
    same(FC.run_fit(lib, bufs, part, slots, False, False, max_iters=8, host=True), whole, "fit", n)
