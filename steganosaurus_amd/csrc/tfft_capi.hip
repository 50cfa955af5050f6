// tfft_capi.hip -- context management and the C ABI of libturtlefft_hip.so
// (include/turtlefft_hip.h).  Host C++ only; all device work is in
// tfft_kernels.hip, tfft_stats.hip, tfft_exact.hip and tfft_audit64.hip.  There is deliberately no CPU fallback in this file: every
// entry point that computes needs a live gfx950 context.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <complex>
#include <initializer_list>
#include <map>
#include <tuple>
#include <new>
#include <vector>

#include "tfft_kernels.h"

extern "C" void tfft_internal_radius_bounds(double lo, double hi, uint64_t* s_lo, uint64_t* s_hi, int* empty);
// host view of the capacity kernel's threshold transform (tests/test_host.py checks it against the reference's compare)
extern "C" float tfft_internal_mag2_threshold(double thr) { return tfft::mag2_threshold(thr); }

namespace {

using namespace tfft;

int next_pow2(int v) { int p = 1; while (p < v) p <<= 1; return p; }        // S:369
int ilog2i(int n) { int l = 0; while ((1 << l) < n) l++; return l; }

struct Slot {     // geometry of one resident image; its buffers are slices of the context pools
    int W = 0, H = 0, PW = 0, PH = 0, PWi = 0, center = 0;
    bool has_spec = false;
    const uint8_t* rgb_src = nullptr;     // device image the last single-image forward of this slot read (tfft_lowfreq_mag reads it again)
};

struct ColPlan { bool direct; int log_n1, log_n2; bool fused_fwd; };

}  // namespace

struct tfft_ctx {
    int device = 0;
    int max_w = 0, max_h = 0, n_slots = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    hipEvent_t ev_t0 = nullptr, ev_t1 = nullptr;
    int last_hip = 0;
    size_t dev_bytes = 0;
    std::vector<Slot> slots;
    // pools, slot i = slice i (fixed strides so that a run of slots is one batched launch)
    size_t img_stride_b = 0;      // bytes between slots in img_pool
    size_t slot_stride = 0;       // float2 elements between slots in spec_pool / tmp_pool
    size_t cand_stride = 0;       // unsigned elements per (slot, plane) in cand_pool
    uint8_t* img_pool = nullptr;
    float2* spec_pool = nullptr;
    float2* tmp_pool = nullptr;
    unsigned* cand_pool = nullptr;
    int stats_prio = 1;                   // the statistics' side stream at the lowest stream priority
    int stats_tile = 1;                   // batched delta embeds run the statistics' bracket pass inside the last forward column step and never store
                                          // the spectrum or |F|^2 (TFFT_STATS_TILE=0: |F|^2 planes + the statistics kernels over them, round 2's default)
    int embed_tile_fuse = 1;              // batched delta embeds with in-step statistics: that step also embeds and runs the first inverse step on the tile it
                                          // holds (COLS_STAT_EMBED).  TFFT_EMBED_TILE_FUSE=0: two launches; 1: launches of >= 2^24 bins; 2: wherever COLS_STAT runs
    int last_embed_path[4] = {0, 0, 0, 0};      // tfft_embed_plan_info: the EmbedPath of the last embed chunk (delta, stats, tile_fuse, side)
    int stats_tile_step_forced = 0;
    int stats_tile_step = 8;              // every 8th column tile is the sample (TFFT_STATS_TILE_STEP)
    float2* col0_pool = nullptr;          // [n_slots*3*max_ph] the packed column 0 of batched embeds that store |F|^2 planes (ColParams::st_col0)
    int stats_skew = 0;                   // test hook (TFFT_STATS_SKEW): brackets moved by this many buckets -- the fast path fails, the fallbacks run
    SelectState* sel = nullptr;           // [n_slots*3]
    float* med = nullptr;                 // [n_slots*3]
    unsigned* partial = nullptr;          // [n_slots*3*TFFT_STAT_MAX_BLOCKS + n_slots]
    float* amb = nullptr;                 // [n_slots*3*TFFT_AMB_CAP] |F|^2 of the bins the bracket pass could not decide
    unsigned long long* usable = nullptr; // [n_slots]
    // exact medians / capacity of the single-image calls (tfft_exact.hip): candidate lists, counters, fp64 values
    int exact_stats = 1;                  // TFFT_EXACT_STATS=0: tfft_medians / tfft_capacity return the fp32 spectrum's own statistics
    ExactCand* ex_cand = nullptr; double2* ex_val = nullptr; unsigned long long* ex_below = nullptr; unsigned* ex_n = nullptr;
    std::map<int, double2*> ex_table;     // PW -> exp(2 pi i j/PW) in fp64
    int ex_last[3] = {0, 0, 0};           // diagnostics: candidates evaluated per plane by the last exact call (0: fp32 result returned)
    int* err = nullptr;                   // sticky bin-range flag
    uint8_t* trash = nullptr;             // 8 KiB nobody reads: target of the unpredicated list stores of lanes without an entry (ColParams::trash)
    int* last_row = nullptr;              // device scalars of k_bins_last_row, one per compute stream
    // spectrum-free extraction (k_fft_cols<..., COLS_READ>): the bin list bucketed by column tile, per compute stream
    struct TileBuckets { float2* fl = nullptr; uint8_t* pb = nullptr; uint64_t fl_cap = 0;      /* delta embedding: values of the listed bins, n_slots x n (ColParams::em_fl) */
                         unsigned* cnt = nullptr; unsigned* off = nullptr; TileBin* ent = nullptr; uint64_t cap = 0; int nb_cap = 0;
                         // what the buckets / the last-row scalar currently describe (tfft_bins_register_dev: reused while the registered list is the one passed in)
                         const void* built_for = nullptr; uint64_t built_n = 0; int built_ph = 0, built_pw = 0, built_g = 0; const void* built_index = nullptr; bool built_bad = false;
                         const void* row_for = nullptr; uint64_t row_n = 0; int row_ph = 0, row_pw = 0;
                         float2* jp = nullptr; uint64_t jp_cap = 0; uint64_t jp_for = 0;      /* the phase options' jitter in bucket order (ColParams::em_jp), gathered for ph_version jp_for */
                       } tb[2];
    const void* reg_bins = nullptr; uint64_t reg_n = 0;      // tfft_bins_register_dev
    int embed_delta = 1;                  // batched embeds: stego = cover + IFFT(F' - F) (TFFT_EMBED_DELTA=0: write F' into the spectrum and invert it)
    int tile_read = 1;                    // TFFT_TILE_READ=0: row-limited spectrum + k_read always; 1: tile read for chunks of >= 8 images; 3: always; 2: always, with the global-atomic bucket build
    hipStream_t stream2 = nullptr;        // TFFT_STREAMS=2: second half of a batch chunk runs here, concurrently
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    // delta embedding leaves the statistics off the critical path (nothing downstream reads the medians): they run on a stream of
    // their own beside the inverse transform -- a read-only pass next to a write-only one (TFFT_STATS_ASYNC=0: in line)
    hipStream_t stream_stats[2] = {nullptr, nullptr};
    hipEvent_t ev_stats_fork[2] = {nullptr, nullptr}, ev_stats_join[2] = {nullptr, nullptr};
    int stats_async = 1;
    int stats_m2 = 1;                     // batched delta embeds store |F|^2 (half the bytes) for the statistics instead of the spectrum nobody else reads (TFFT_STATS_M2=0)
    int n_streams = 1;
    int n_cus = 0, collect_resident = 0;  // grid sizing of the full median pass: fill every CU to the same depth
    uint32_t* bit_index = nullptr;        // tfft_set_bit_index: bins[i] carries stream bit bit_index[i]
    uint64_t bit_index_n = 0;
    // tfft_set_phase_options: the batched calls' jitter (device, stream order, ph_n floats; nullptr = none) and adaptive alpha.
    // ph_version changes with every call of the setter (0: never set), so that bucket-order copies and cached sequences can tell
    float* ph_jit = nullptr;
    uint64_t ph_n = 0;
    int ph_adaptive = 0;
    uint64_t ph_version = 0;
    std::map<int, float2*> tw;            // N -> table exp(+2 pi i j/N), j < N
    std::map<std::tuple<int, int, int, int>, float2*> dc;   // (valid, N, center, kind) -> DC-removal table, see get_dc_table
    float dc_bias = 128.0f;               // constant taken out of the pixels before the forward transform and put back analytically (see
                                          // get_dc_table; both directions).  ON by default: it is what keeps every coefficient within the
                                          // 1e-4 relative tolerance on padded images.  TFFT_DC_BIAS=0 switches it off (A/B measurements only)
    uint8_t* sio_hdr = nullptr; uint8_t* sio_pay = nullptr; int* sio_status = nullptr; uint64_t sio_plen = 0;      // host-buffer stream pipelines
    uint8_t* stream_bits = nullptr; unsigned* stream_plen = nullptr; size_t stream_cap = 0;   // tfft_*_stream_batch_dev: expanded / raw bits of a chunk
    void* stage_bins = nullptr; void* stage_bits = nullptr; void* stage_jit = nullptr; void* stage_out = nullptr;
    size_t stage_cap = 0;
    hipStream_t s_in = nullptr, s_out = nullptr;      // host-buffer pipeline (created on first use)
    hipEvent_t ev_in[4] = {}, ev_comp[4] = {}, ev_out[4] = {};
    uint8_t* out_pool = nullptr;
    int cols_direct_max_log = 8;          // PH <= 256: one column pass; taller: two-step N1 x N2 (a direct 512 pass reaches 1.8-3.4 TB/s, the two steps 5-6)
    int cols_force_log_n1 = -1;
    int cols_tiles_per_block = 8;
    int cols_tiles_forced = 0;            // TFFT_COLS_TILES given: it also rules the COLS_EMIT step (default there: 2 tiles per workgroup up to L = 256, r3h A/B: 0.601 vs 0.630 ms per 32 x 1080p launch)
    int cols_tiles_embed = 0;             // delta embedding: tiles per workgroup of the first inverse step; 0 = 8 for columns up to 256, 2 from 512 on
                                          // (round 3 A/B, gpurun_out/r3h, per 32 x 1080p launch: 0.490 / 0.437 / 0.404 / 0.394 ms with 2 / 4 / 8 / 16; per 8 x 4K: 0.563 / 0.501 / 0.511 / 0.518 with 1 / 2 / 4 / 8)
    int cols_tiles_stat = 16;             // COLS_STAT: tiles per workgroup (nothing is stored: as the tile-resident read; r4d A/B 1080p x 32: 2.048 / 2.024 / 2.000 / 1.997 ms per embed with 2 / 4 / 8 / 16)
    int cols_tiles_read = 16;             // the tile-resident read walks longer runs (A/B: 0.422 vs 0.455 ms per 32x1080p launch; the storing steps prefer 8)
    int median_force_fallback = 0;
#ifndef TFFT_NO_GRAPHS
    // launch-bound calls (a few images): the launch sequence of a batch call is captured once into a hipGraph, keyed by every
    // argument, and replayed.  state 1 = seen once (the next call captures), exec != nullptr = replay
    struct GraphEntry { hipGraphExec_t exec = nullptr; int state = 0; };
    std::map<std::vector<uint64_t>, GraphEntry> graphs;
#endif
    int stats_fail_once = 0;              // TFFT_STATS_FAIL_ONCE (test hook)
    bool stats_dirty = false;             // a statistics launch sequence broke off midway: the select state (histograms left zero by convention) is cleared before the next one
    bool graphs_stale = false;            // the shared bucket buffers were rebuilt for another list: captured sequences that left the build out must go
    int graph_max_images = 0;             // TFFT_GRAPHS=n: replay calls of up to n images.  Off by default: measured 5 % SLOWER than plain
                                          // launches (0.283 vs 0.267 ms per 1080p round trip) -- a single image is bound by the GPU-side
                                          // latency of its dependent kernels, which a graph does not shorten
    int stats_fused = 1;                  // TFFT_STATS_FUSED=0: capacity as its own pass after the medians (A/B)
    int stats_compact = 1;                // TFFT_STATS_COMPACT=0: the 16-launch statistics pipeline also for small planes (A/B)
    int fuse = 1;
    int fuse_wide = 1;
    int fuse_live = 1;                    // TFFT_FUSE_LIVE=0: the fused forward kernel with a wave (pair) and a slab for all 8 rows of a group (A/B)
    // the fitted embed (tfft_embed_stream_batch_fit*): per bucket entry of a chunk the corrected delta and the margin; per image the
    // count partials, the counts, and the host form's iteration / wrong-bit outputs
    float2* fit_d = nullptr; float* fit_mu = nullptr; uint64_t fit_cap = 0;
    unsigned* fit_part = nullptr; unsigned* fit_cnt = nullptr; int32_t* fit_iters = nullptr; uint32_t* fit_wrong = nullptr;
    // tfft_set_batch_exact: the batched embeds' usable_out settled in fp64 like tfft_capacity.  The device buffers are
    // allocated when the mode is first turned on, for n_slots images; bx_state holds the per-image states of the last call that filled usable_out
    int bx_mode = 0; uint64_t bx_guard = 64; int bx_trace = 0;      // TFFT_BATCH_EXACT_TRACE=1: one line per settled chunk on stderr (tools/exact_cost.py)
    std::vector<int32_t> bx_state; int bx_last_n = 0;
    ExactWin* bx_win = nullptr; ExactCandB* bx_cand = nullptr; unsigned long long* bx_below = nullptr; unsigned* bx_n = nullptr;
    unsigned* bx_idx = nullptr; ExactGroup* bx_grp = nullptr; double2* bx_part = nullptr; ExactVal* bx_val = nullptr; size_t bx_part_cap = 0, bx_val_cap = 0;
    // the analysis scratch (tfft_phase_hist_batch*, tfft_quality_batch*, tfft_channel_batch, tfft_robustness_batch*, tfft_spam_batch): what one
    // chunk of the running call needs beside the slots -- partials, attacked images, decode outputs, the host forms' staged images and
    // results.  One buffer, grown on demand (ensure_analysis), laid out afresh by every call (Carve); nothing in it outlives its call
    void* an_buf = nullptr; size_t an_cap = 0;

    uint8_t* img(int i) const { return img_pool + (size_t)i * img_stride_b; }
    float2* spec(int i) const { return spec_pool + (size_t)i * slot_stride; }
    float2* tmp(int i) const { return tmp_pool + (size_t)i * slot_stride; }
};

namespace {

#define HIPCHK(ctx, call)                                  \
    do {                                                   \
        hipError_t e_ = (call);                            \
        if (e_ != hipSuccess) { (ctx)->last_hip = (int)e_; return TFFT_E_HIP; } \
    } while (0)

int dev_alloc(tfft_ctx* c, void** p, size_t bytes) {
    if (hipMalloc(p, bytes) != hipSuccess) { *p = nullptr; return TFFT_E_NOMEM; }
    c->dev_bytes += bytes;
    return TFFT_OK;
}

int get_twiddles(tfft_ctx* c, int n, const float2** out) {
    auto it = c->tw.find(n);
    if (it != c->tw.end()) { *out = it->second; return TFFT_OK; }
    std::vector<float2> h((size_t)n);
    for (int j = 0; j < n; j++) {
        const double a = 2.0 * M_PI * (double)j / (double)n;
        h[j] = make_float2((float)cos(a), (float)sin(a));
    }
    float2* d = nullptr;
    int rc = dev_alloc(c, (void**)&d, sizeof(float2) * (size_t)n);
    if (rc) return rc;
    HIPCHK(c, hipMemcpy(d, h.data(), sizeof(float2) * (size_t)n, hipMemcpyHostToDevice));
    c->tw[n] = d;
    *out = d;
    return TFFT_OK;
}

// n = images in the launch the plan is for (the fused 4096-wide kernels only pay off with more than one: 1536 workgroups of
// 1024 threads leave the tail of a single image on a few CUs -- measured 0.85 vs 0.82 ms per 4K round trip)
ColPlan plan_cols(const tfft_ctx* c, int PH, int PWi, int n) {
    const int l = ilog2i(PH);
    ColPlan p;
    p.fused_fwd = false;
    if (c->fuse && c->cols_force_log_n1 < 0 && l >= 7 &&
        ((PWi == 2048 && l - 3 <= 9) || (PWi == 4096 && l - 3 <= 9 && (c->fuse_wide >= 2 || (c->fuse_wide == 1 && n >= 2))))) {
        // rows + first column step in one kernel (k_rowcol_fwd): PH = 8 * N2.  2048 wide: one wave per row; 4096 wide: two waves
        // per row, 1024-thread workgroups, for launches of two or more images (TFFT_FUSE_WIDE=0: never, 2: always)
        p.direct = false; p.log_n1 = 3; p.log_n2 = l - 3; p.fused_fwd = true;
        return p;
    }
    if (l <= c->cols_direct_max_log && c->cols_force_log_n1 < 0) { p.direct = true; p.log_n1 = 0; p.log_n2 = l; return p; }
    p.direct = false;
    int l1 = (c->cols_force_log_n1 >= 0) ? c->cols_force_log_n1 : l / 2;
    if (l1 < 1) l1 = 1;
    if (l1 > l - 1) l1 = l - 1;
    if (l - l1 > 9) l1 = l - 9;
    p.log_n1 = l1; p.log_n2 = l - l1;
    return p;
}

int set_geometry(tfft_ctx* c, Slot& s, int w, int h, int center) {
    if (w < 1 || h < 1) return TFFT_E_INVALID;
    if (w > c->max_w || h > c->max_h) return TFFT_E_TOO_LARGE;
    s.W = w; s.H = h; s.PW = next_pow2(w); s.PH = next_pow2(h);
    s.PWi = s.PW < 2 ? 2 : s.PW;          // the real<->half-complex row transform needs an even length
    s.center = center ? 1 : 0;
    if (s.PWi > TFFT_MAX_DIM || s.PH > TFFT_MAX_DIM) return TFFT_E_TOO_LARGE;
    return TFFT_OK;
}

// The pipeline as addressable stages, each ONE batched launch over slots [s0, s0+n) of equal geometry
// (also used by tfft_profile_stage).
//   forward : ROWS_FWD (u8 -> tmp), COLS_FWD_A (tmp -> tmp | spec), COLS_FWD_B (tmp -> spec, two-step only)
//   inverse : COLS_INV_A (spec -> tmp), COLS_INV_B (tmp -> tmp, two-step only), ROWS_INV (tmp -> u8)
enum Stage { ROWS_FWD = 0, COLS_FWD_A = 1, COLS_FWD_B = 2, EMBED = 3, COLS_INV_A = 4, COLS_INV_B = 5, ROWS_INV = 6,
             READ = 7, MEDIANS = 8, CAPACITY = 9,
             COLS_FWD_READ = 10,      // the final forward column step as extraction runs it (rows above the bin list's last row not stored)
             N_STAGES = 11 };

int get_dc_table(tfft_ctx* c, int valid, int N, int center, int kind, double scale, const float2** out);
void invalidate_graphs(tfft_ctx* c);      // cached launch sequences hold raw device pointers: dropped whenever a buffer is reallocated

// Quiesce, then free: before a device buffer goes away that enqueued work or a cached sequence may still name, both compute streams are
// drained and the cached sequences dropped.  (Every batched call joins stream2 into stream before it returns: the second wait is free.)
int quiesce(tfft_ctx* c) {
    const hipError_t e1 = hipStreamSynchronize(c->stream);
    const hipError_t e2 = c->stream2 ? hipStreamSynchronize(c->stream2) : hipSuccess;
    invalidate_graphs(c);
    if (e1 != hipSuccess || e2 != hipSuccess) { c->last_hip = (int)(e1 != hipSuccess ? e1 : e2); return TFFT_E_HIP; }
    return TFFT_OK;
}
// the growth policy of the buffers sized by a call's arguments: a quarter of headroom, so that slowly growing requests do not reallocate each time
inline uint64_t grown(uint64_t n, uint64_t pad) { return n + n / 4 + pad; }
// the buffers of one group replaced (the owner records capacity 0 before and the new one after: a group that failed grows again next time)
struct Regrow { void** p; size_t bytes; };
int regrow(tfft_ctx* c, std::initializer_list<Regrow> bufs) {
    int rc = quiesce(c);
    if (rc) return rc;
    for (const Regrow& b : bufs) { (void)hipFree(*b.p); *b.p = nullptr; }
    for (const Regrow& b : bufs) if (dev_alloc(c, b.p, b.bytes)) return TFFT_E_NOMEM;
    return TFFT_OK;
}

// How a launch sequence wants the outer column steps and the inverse row kernel to run: handed down explicitly per call (until round 3
// these were pointers parked in the context around a call -- to stack objects, and left dangling by any early return in between).
// A step's parameter object carries the fields its mode reads (tfft_kernels.h: ColParams says which); the geometry, the DC tables, the
// scratch line and tiles_per_block are the stage's own (last_forward_params, first_inverse_params)
struct StageMode {
    int fwd_mode = COLS_PLAIN;             // the last forward column step: COLS_PLAIN (fwd: the statistics' sample or the gate, or nullptr),
    const ColParams* fwd = nullptr;        // COLS_ROWLIMIT, COLS_READ, COLS_EMIT or COLS_STAT
    float2* fwd_out_override = nullptr;    // ... and its output buffer
    int inv_mode = COLS_PLAIN;             // the first inverse column step: COLS_PLAIN (inv: nullptr), COLS_EMBED or COLS_EMBED_D (delta embedding)
    const ColParams* inv = nullptr;
    bool walks = false;                    // the lists are one walk per image (ColStep::walks).  One flag for both steps: a caller fills
                                           // in the step its launch sequence runs in a bucket mode, and the flag goes with that step (a COLS_PLAIN
                                           // or COLS_ROWLIMIT step has no lists: launch_cols rejects it with the flag set)
    const uint8_t* inv_cover = nullptr;    // the inverse row kernel adds its transform to these cover pixels (delta embedding)
    bool inv_first_done = false;           // the first inverse column step ran inside the last forward one (COLS_STAT_EMBED, which left its output in `spec`)
    bool inv_via_spec = false;             // delta embedding: the inverse keeps its intermediate in `spec` (nothing reads F there), so `tmp` -- the
                                           // input of the last forward step -- survives for the gated fallback of the in-kernel statistics
};

// a column step's parameters: the fields of `from` (or none) + what every step of slot geometry s shares
static ColParams col_params(const tfft_ctx* c, const Slot& s, const ColParams* from) {
    ColParams cp = from ? *from : ColParams{};
    cp.M = s.PWi / 2; cp.PH = s.PH; cp.plane_stride = (size_t)s.PH * cp.M; cp.img_stride = c->slot_stride;
    cp.tiles_per_block = c->cols_tiles_per_block;
    return cp;
}
static int dc_tables(tfft_ctx* c, const Slot& s, ColParams& cp) {
    if (c->dc_bias == 0.0f) return TFFT_OK;
    int rc = get_dc_table(c, s.H, s.PH, s.center, 0, (double)c->dc_bias, &cp.dc_ah);
    if (!rc) rc = get_dc_table(c, s.W, s.PWi, s.center, 1, 1.0, &cp.dc_aw);
    return rc;
}
// the last forward column step: the only one of a direct plan, else for every k1 the length-N2 FFT over rows k1*N2+n2 -> rows k1+N1*k2
static int last_forward_params(tfft_ctx* c, const Slot& s, const ColPlan& pl, const StageMode& md, ColParams& cp) {
    const int N1 = 1 << pl.log_n1, N2 = 1 << pl.log_n2;
    cp = col_params(c, s, md.fwd);
    if (pl.direct) { cp.G = 1; cp.in_a = 1; cp.in_b = 0; cp.out_a = 1; cp.out_b = 0; cp.in_rows = s.H; }
    else { cp.G = N1; cp.in_a = 1; cp.in_b = N2; cp.out_a = N1; cp.out_b = 1; cp.in_rows = s.PH; }
    cp.out_rows = s.PH; cp.tw_out = 0;
    switch (md.fwd_mode) {
        case COLS_PLAIN:
            if (cp.tile_step > 1) cp.tiles_per_block = cp.hist_sel ? 2 : 1;      // the sample: an eighth of the tiles; few per workgroup keep the grid wide
            break;
        case COLS_READ: cp.trash = c->trash; cp.tiles_per_block = c->cols_tiles_read; break;
        case COLS_EMIT: case COLS_STAT: case COLS_STAT_EMBED:
            cp.trash = c->trash;
            // (the phase options belong to COLS_EMBED, whose object this may be -- and to the step that embeds in the same visit)
            if (md.fwd_mode != COLS_STAT_EMBED) cp.em_jp = nullptr;
            cp.em_med = nullptr; cp.em_alpha = 0.f;
            if (!c->cols_tiles_forced && pl.log_n2 <= 8) cp.tiles_per_block = 2;
            if (stat_mode(md.fwd_mode) && c->cols_tiles_stat) cp.tiles_per_block = c->cols_tiles_stat;
            break;
    }
    return dc_tables(c, s, cp);
}
// the first inverse column step: the only one of a direct plan, else for every k1 the length-N2 inverse over rows k1+N1*k2 -> rows
// k1*N2+n2, times w^-(n2*k1)
static int first_inverse_params(tfft_ctx* c, const Slot& s, const ColPlan& pl, const StageMode& md, ColParams& cp) {
    const int N1 = 1 << pl.log_n1, N2 = 1 << pl.log_n2;
    cp = col_params(c, s, md.inv);
    if (pl.direct) { cp.G = 1; cp.in_a = 1; cp.in_b = 0; cp.out_a = 1; cp.out_b = 0; cp.out_rows = s.H; cp.tw_out = 0; }
    else { cp.G = N1; cp.in_a = N1; cp.in_b = 1; cp.out_a = 1; cp.out_b = N2; cp.out_rows = s.PH; cp.tw_out = 1; }
    cp.in_rows = s.PH;
    if (!embed_mode(md.inv_mode)) return dc_tables(c, s, cp);      // (the tiles of a delta embed hold F' - F: no DC term to take out)
    cp.trash = c->trash;
    cp.tiles_per_block = c->cols_tiles_embed ? c->cols_tiles_embed : (pl.log_n2 >= 9 ? 2 : 16);
    return TFFT_OK;
}

int enqueue_fft_stage(tfft_ctx* c, int s0, int n, int stage, const uint8_t* rgb_in, uint8_t* rgb_out, hipStream_t st, const StageMode& md = StageMode()) {
    const Slot& s = c->slots[s0];
    const int M = s.PWi / 2;
    const float2 *tw_w, *tw_h;
    int rc = get_twiddles(c, s.PWi, &tw_w); if (rc) return rc;
    rc = get_twiddles(c, s.PH, &tw_h); if (rc) return rc;
    const ColPlan pl = plan_cols(c, s.PH, s.PWi, n);
    const int N2 = 1 << pl.log_n2;
    float2 *spec = c->spec(s0), *tmp = c->tmp(s0);
    float2* inv_mid = md.inv_via_spec ? spec : tmp;      // where the inverse keeps its intermediate
    ColParams cp = col_params(c, s, nullptr);
    auto last_forward = [&]() -> int {
        rc = last_forward_params(c, s, pl, md, cp); if (rc) return rc;
        HIPCHK(c, launch_cols(tmp, md.fwd_out_override ? md.fwd_out_override : spec, tw_h, cp, ColStep{pl.log_n2, +1, md.fwd_mode, md.walks}, 3 * n, st));
        return TFFT_OK;
    };
    switch (stage) {
        case ROWS_FWD: {
            RowParams rp{s.W, s.H, s.PWi, s.PH, s.center, 0.f, c->slot_stride, c->dc_bias, nullptr};
            // rows + column step A; when some rows of the groups are padding, by the live-rows-only kernel (a full-height image has none)
            if (pl.fused_fwd && c->fuse_live && s.H < s.PH) HIPCHK(c, launch_rowcol_fwd_live(rgb_in, tmp, tw_w, tw_h, rp, n, st));
            else if (pl.fused_fwd) HIPCHK(c, launch_rowcol_fwd(rgb_in, tmp, tw_w, tw_h, rp, n, st));
            else HIPCHK(c, launch_rows_fwd(rgb_in, tmp, tw_w, rp, n, st));
            return TFFT_OK;
        }
        case COLS_FWD_A:
            if (pl.fused_fwd) return TFFT_OK;       // done inside ROWS_FWD
            if (pl.direct) return last_forward();
            // for every n2: length-N1 FFT over rows n1*N2+n2, times w^(n2*k1), in place
            cp.G = N2; cp.in_a = N2; cp.in_b = 1; cp.out_a = N2; cp.out_b = 1; cp.in_rows = s.H; cp.out_rows = s.PH; cp.tw_out = 1;
            HIPCHK(c, launch_cols(tmp, tmp, tw_h, cp, ColStep{pl.log_n1, +1, COLS_PLAIN, false}, 3 * n, st));
            return TFFT_OK;
        case COLS_FWD_B:
            return pl.direct ? TFFT_OK : last_forward();
        case COLS_INV_A:
            rc = first_inverse_params(c, s, pl, md, cp); if (rc) return rc;
            HIPCHK(c, launch_cols(spec, inv_mid, tw_h, cp, ColStep{pl.log_n2, -1, md.inv_mode, md.walks}, 3 * n, st));
            return TFFT_OK;
        case COLS_INV_B:
            if (pl.direct || pl.fused_fwd) return TFFT_OK;      // fused: done inside ROWS_INV
            // for every n2: length-N1 inverse over rows k1*N2+n2 -> rows n1*N2+n2 (< H only), in place
            cp.G = N2; cp.in_a = N2; cp.in_b = 1; cp.out_a = N2; cp.out_b = 1; cp.in_rows = s.PH; cp.out_rows = s.H; cp.tw_out = 0;
            HIPCHK(c, launch_cols(inv_mid, inv_mid, tw_h, cp, ColStep{pl.log_n1, -1, COLS_PLAIN, false}, 3 * n, st));
            return TFFT_OK;
        case ROWS_INV: {
            RowParams rp{s.W, s.H, s.PWi, s.PH, s.center, (float)(1.0 / ((double)M * (double)s.PH)), c->slot_stride, c->dc_bias, nullptr};
            if (md.inv_cover) { rp.cover = md.inv_cover; rp.bias = 0.f; }      // delta embedding: the transform of F' - F has no DC term to give back
            if (md.inv_via_spec && !embed_mode(md.inv_mode)) return TFFT_E_INVALID;      // only the delta inverse reads nothing from `spec`
            if (pl.fused_fwd) HIPCHK(c, launch_colrow_inv(inv_mid, rgb_out, tw_w, rp, n, st));       // column step B' + rows
            else HIPCHK(c, launch_rows_inv(inv_mid, rgb_out, tw_w, rp, n, st));
            return TFFT_OK;
        }
        default: return TFFT_E_INVALID;
    }
}

// forward: rows (u8 -> tmp) then columns (tmp -> spec) for slots [s0, s0+n); images contiguous at rgb_dev
int enqueue_forward(tfft_ctx* c, int s0, int n, const uint8_t* rgb_dev, hipStream_t st, const StageMode& md = StageMode()) {
    for (int stage : {ROWS_FWD, COLS_FWD_A, COLS_FWD_B}) {
        int rc = enqueue_fft_stage(c, s0, n, stage, rgb_dev, nullptr, st, md);
        if (rc) return rc;
    }
    for (int i = 0; i < n; i++) { c->slots[s0 + i].has_spec = true; c->slots[s0 + i].rgb_src = nullptr; }
    return TFFT_OK;
}

// inverse: columns (spec -> tmp, only rows < H kept) then rows (tmp -> u8)
int enqueue_inverse(tfft_ctx* c, int s0, int n, uint8_t* rgb_out_dev, hipStream_t st, const StageMode& md = StageMode()) {
    for (int stage : {COLS_INV_A, COLS_INV_B, ROWS_INV}) {
        if (stage == COLS_INV_A && md.inv_first_done) continue;
        int rc = enqueue_fft_stage(c, s0, n, stage, nullptr, rgb_out_dev, st, md);
        if (rc) return rc;
    }
    for (int i = 0; i < n; i++) c->slots[s0 + i].has_spec = false;
    return TFFT_OK;
}

// DC removal.  A DC-heavy image (every photograph) makes the partial sums of an fp32 FFT as large as the mean
// term itself, and the rows / columns through the DC bin -- and the bins beside them, which sit on its sidelobes
// when the image is padded -- come out with an ABSOLUTE error of ~1 ulp of that term (the fp64 audit transform
// measured 1e-4..4e-4 of the spectrum's rms on the axes, 1.5e-4 relative beside them).  So the row kernels subtract
// a constant c from every pixel (s*(b - c), s = the centring sign) and the LAST forward column step adds the exact
// transform of s*c*rect(W x H) back:  c * A_H(y) * A_W(x),  A_N(k) = sum_{n < valid} sigma^n exp(+2 pi i n k/N),
// a geometric series evaluated in fp64 here.  kind 0: c*A_H(y), y < PH.  kind 1: A_W(x), x < M, entry 0 packed as
// A_W(0) + i*A_W(M) like the spectrum's column 0.
static std::complex<double> dc_series(int k, int valid, int N, int center) {
    double th = 2.0 * M_PI * (double)k / (double)N + (center ? M_PI : 0.0);
    th = fmod(th, 2.0 * M_PI);
    const double sh = sin(0.5 * th);
    if (fabs(sh) < 1e-14) return std::complex<double>((double)valid, 0.0);
    const double mag = sin(0.5 * th * valid) / sh, ph = 0.5 * th * (valid - 1);
    return std::complex<double>(mag * cos(ph), mag * sin(ph));
}
int get_dc_table(tfft_ctx* c, int valid, int N, int center, int kind, double scale, const float2** out) {
    const auto key = std::make_tuple(valid, N, center ? 1 : 0, kind);
    auto it = c->dc.find(key);
    if (it != c->dc.end()) { *out = it->second; return TFFT_OK; }
    const int n = (kind == 0) ? N : (N / 2 > 0 ? N / 2 : 1);
    std::vector<float2> h((size_t)n);
    for (int k = 0; k < n; k++) {
        std::complex<double> a = dc_series(k, valid, N, center);
        if (kind == 1 && k == 0) a += std::complex<double>(0.0, 1.0) * dc_series(N / 2, valid, N, center);
        a *= scale;
        h[k] = make_float2((float)a.real(), (float)a.imag());
    }
    float2* d = nullptr;
    int rc = dev_alloc(c, (void**)&d, sizeof(float2) * (size_t)n);
    if (rc) return rc;
    HIPCHK(c, hipMemcpy(d, h.data(), sizeof(float2) * (size_t)n, hipMemcpyHostToDevice));
    c->dc[key] = d;
    *out = d;
    return TFFT_OK;
}

EmbedParams embed_params(const tfft_ctx* c, const Slot& s, uint64_t n, double alpha, int adaptive, const double med[3],
                         bool has_jitter) {
    EmbedParams p{};
    p.n = n; p.PH = s.PH; p.PW = s.PW;
    p.adaptive = adaptive ? 1 : 0;
    p.generic = (adaptive || has_jitter || !(alpha > 0.0 && alpha < M_PI)) ? 1 : 0;
    p.cos_a = (float)cos(alpha); p.sin_a = (float)sin(alpha);
    p.alpha = alpha;
    for (int i = 0; i < 3; i++) p.med[i] = med ? med[i] : 0.0;
    p.img_stride = c->slot_stride;
    p.bit_index = c->bit_index;            // callers check index_ok(c, n) first
    p.limit = n;
    return p;
}
// a bit index, once set, must describe exactly the bin list it is used with
static inline bool index_ok(const tfft_ctx* c, uint64_t n) { return !c->bit_index || c->bit_index_n == n; }
// ... and so must the jitter of the phase options (batched calls only)
static inline bool phase_ok(const tfft_ctx* c, uint64_t n) { return !c->ph_jit || c->ph_n == n; }
// what a cached launch sequence of a batched call depends on besides its arguments
static void phase_key(const tfft_ctx* c, std::vector<uint64_t>& key) {
    key.push_back((uint64_t)(uintptr_t)c->ph_jit); key.push_back(c->ph_n); key.push_back((uint64_t)c->ph_adaptive); key.push_back(c->ph_version);
}

CapParams cap_params(const tfft_ctx* c, const Slot& s, double rmin, double rmax) {
    CapParams p{};
    p.PH = s.PH; p.PW = s.PW; p.PWi = s.PWi; p.img_stride = c->slot_stride;
    const int mn = s.PH < s.PW ? s.PH : s.PW;
    const double lo = rmin * mn, hi = rmax * mn;        // S:1003
    uint64_t a, b; int empty;
    tfft_internal_radius_bounds(lo, hi, &a, &b, &empty);
    p.s_lo = a; p.s_hi = b;
    if (empty) { p.bw = p.bh = 0; return p; }
    double lim = floor(hi) + 1.0;
    p.bw = (int)(lim < (double)s.PW ? lim : (double)s.PW);
    p.bh = (int)(lim < (double)s.PH ? lim : (double)s.PH);
    return p;
}

// medians of slots [s0, s0+n); cap != nullptr: also their capacities (S:998-1008 with thr = magmin * median) -> usable[0..n)
// m2: the slots hold |F|^2 planes + packed columns 0 (stats_m2_applies) instead of the spectrum
// The select kernels leave SelectState.hist zero behind them instead of clearing it in front (one launch less per call): a sequence that
// breaks off midway -- a failed launch, an error on the side stream -- would hand dirty histograms to every later call on those slots.
// Whoever sees such a failure marks the context; the next statistics sequence clears the whole state first.
static int stats_clean_if_dirty(tfft_ctx* c, hipStream_t st) {
    if (!c->stats_dirty) return TFFT_OK;
    HIPCHK(c, hipMemsetAsync(c->sel, 0, (size_t)c->n_slots * 3 * sizeof(SelectState), st));
    c->stats_dirty = false;
    return TFFT_OK;
}
// the statistics' buffers of slots [s0, s0+n), capacities -> usable.  (The batch capacity keeps its partial counts and flags in ONE region
// per call: the slots use the start of the pool's share of the compute stream -- s0 is 0 or the second half of a two-stream chunk: shares do
// not overlap for n <= n_slots - s0)
static float2* stat_col0(tfft_ctx* c, int s0) { return c->col0_pool + (size_t)s0 * 3 * c->slots[s0].PH; }
static unsigned* stat_partial(tfft_ctx* c, int s0) { return c->partial + (size_t)s0 * (3 * TFFT_STAT_MAX_BLOCKS + 1); }
static StatBufs stat_bufs(tfft_ctx* c, int s0, unsigned long long* usable) {
    return StatBufs{c->sel + 3 * s0, c->cand_pool + (size_t)3 * s0 * c->cand_stride, c->cand_stride, c->med + 3 * s0,
                    stat_partial(c, s0), c->amb + (size_t)3 * s0 * TFFT_AMB_CAP, usable, stat_col0(c, s0)};
}
static StatOpts stat_opts(const tfft_ctx* c, const CapParams* cap, bool m2) {
    return StatOpts{cap, m2, c->stats_compact, c->median_force_fallback, c->stats_skew, c->n_cus, c->collect_resident};
}
static int enqueue_medians_impl(tfft_ctx* c, int s0, int n, hipStream_t st, const CapParams* cap, unsigned long long* usable, bool m2);
int enqueue_medians(tfft_ctx* c, int s0, int n, hipStream_t st, const CapParams* cap = nullptr, unsigned long long* usable = nullptr, bool m2 = false) {
    int rc = stats_clean_if_dirty(c, st);
    if (!rc) rc = enqueue_medians_impl(c, s0, n, st, cap, usable, m2);
    if (rc) c->stats_dirty = true;
    return rc;
}
static int enqueue_medians_impl(tfft_ctx* c, int s0, int n, hipStream_t st, const CapParams* cap, unsigned long long* usable, bool m2) {
    const Slot& s = c->slots[s0];
    HIPCHK(c, launch_medians(c->spec(s0), s.PH, s.PWi, c->slot_stride, n, stat_bufs(c, s0, usable), stat_opts(c, cap, m2), st));
    return TFFT_OK;
}
// the batched delta embeds with capacity: may the last forward step store |F|^2 instead of the spectrum?
static bool stats_m2_applies(const tfft_ctx* c, const Slot& s, const CapParams& p) {
    return c->stats_m2 && c->stats_fused && c->stats_compact && !c->median_force_fallback && p.bw > 0 &&
           (unsigned long long)s.PH * s.PWi <= TFFT_COMPACT_MAX_BINS;
}

int ensure_stage(tfft_ctx* c, uint64_t n) {
    if (n <= c->stage_cap) return TFFT_OK;
    c->stage_cap = 0;
    const size_t cap = grown(n, 1024);
    int rc = regrow(c, {{&c->stage_bins, cap * sizeof(tfft_bin)}, {&c->stage_bits, cap}, {&c->stage_jit, cap * sizeof(float)}, {&c->stage_out, cap}});
    if (rc) return rc;
    c->stage_cap = cap;
    return TFFT_OK;
}

int check_err_flag(tfft_ctx* c) {
    int flag = 0;
    HIPCHK(c, hipMemcpyAsync(&flag, c->err, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (flag) {
        HIPCHK(c, hipMemsetAsync(c->err, 0, sizeof(int), c->stream));
        return TFFT_E_BIN_RANGE;
    }
    return TFFT_OK;
}

// ---- hipGraph replay of launch-bound batch calls ---------------------------------------------------------------
void invalidate_graphs(tfft_ctx* c) {
#ifndef TFFT_NO_GRAPHS
    for (auto& kv : c->graphs) if (kv.second.exec) (void)hipGraphExecDestroy(kv.second.exec);
    c->graphs.clear();
#else
    (void)c;
#endif
}
inline uint64_t key_bits(double v) { uint64_t u; memcpy(&u, &v, sizeof u); return u; }
inline uint64_t key_bits(const void* p) { return (uint64_t)(uintptr_t)p; }
// enqueue(): the normal launch sequence on c->stream.  after(): the host-side slot state the sequence leaves behind (replays skip
// the host code of enqueue()).  First call with a key: plain launches (every table / buffer the sequence needs is created here,
// outside any capture).  Second call: captured + instantiated + launched.  Later calls: one hipGraphLaunch.
template <class Enqueue, class After>
int with_graph(tfft_ctx* c, int n_images, const std::vector<uint64_t>& key, Enqueue&& enqueue, After&& after) {
#ifndef TFFT_NO_GRAPHS
    if (c->graph_max_images > 0 && n_images > 0 && n_images <= c->graph_max_images && c->n_streams < 2) {
        if (c->graphs.size() > 64 || c->graphs_stale) { invalidate_graphs(c); c->graphs_stale = false; }
        auto& e = c->graphs[key];
        if (e.exec) {
            HIPCHK(c, hipGraphLaunch(e.exec, c->stream));
            return after();
        }
        if (e.state == 1) {
            e.state = 2;            // whatever happens, do not try to capture this key again
            if (hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal) == hipSuccess) {
                const int rc = enqueue();
                hipGraph_t g = nullptr;
                const hipError_t ee = hipStreamEndCapture(c->stream, &g);
                hipGraphExec_t ex = nullptr;
                if (rc == TFFT_OK && ee == hipSuccess && g && hipGraphInstantiate(&ex, g, nullptr, nullptr, 0) == hipSuccess) {
                    (void)hipGraphDestroy(g);
                    c->graphs[key].exec = ex;
                    HIPCHK(c, hipGraphLaunch(ex, c->stream));
                    return after();
                }
                if (g) (void)hipGraphDestroy(g);
                (void)hipGetLastError();
                c->last_hip = 0;
                return enqueue();       // capture refused or broken (nothing ran): plain launches; a genuine error shows up again here
            }
            (void)hipGetLastError();
        } else if (e.state == 0) e.state = 1;
    }
#else
    (void)n_images; (void)key; (void)after;
#endif
    return enqueue();
}

bool slot_ok(const tfft_ctx* c, int slot) { return c && slot >= 0 && slot < c->n_slots; }

}  // namespace

extern "C" {

int tfft_abi_version(void) { return TFFT_ABI_VERSION; }

const char* tfft_strerror(int status) {
    switch (status) {
        case TFFT_OK: return "ok";
        case TFFT_E_INVALID: return "invalid argument";
        case TFFT_E_NO_DEVICE: return "no usable gfx950 HIP device (this library has no CPU fallback)";
        case TFFT_E_TOO_LARGE: return "image larger than the context allows";
        case TFFT_E_NOMEM: return "out of memory";
        case TFFT_E_HIP: return "HIP runtime error";
        case TFFT_E_STATE: return "slot holds no forward spectrum";
        case TFFT_E_EXHAUSTED: return "annulus exhausted";
        case TFFT_E_BIN_RANGE: return "bin outside the grid or on an excluded axis";
        default: return "unknown status";
    }
}

int tfft_create(int device, int max_w, int max_h, int n_slots, tfft_ctx** out) {
    if (!out || max_w < 1 || max_h < 1 || n_slots < 1 || n_slots > 1024) return TFFT_E_INVALID;
    *out = nullptr;
    int pw = next_pow2(max_w), ph = next_pow2(max_h);
    if (pw < 2) pw = 2;
    if (pw > TFFT_MAX_DIM || ph > TFFT_MAX_DIM) return TFFT_E_TOO_LARGE;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return TFFT_E_NO_DEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return TFFT_E_NO_DEVICE;
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0 && !getenv("TFFT_ALLOW_OTHER_ARCH")) return TFFT_E_NO_DEVICE;
    if (hipSetDevice(device) != hipSuccess) return TFFT_E_NO_DEVICE;
    tfft_ctx* c = new (std::nothrow) tfft_ctx();
    if (!c) return TFFT_E_NOMEM;
    c->device = device; c->max_w = max_w; c->max_h = max_h; c->n_slots = n_slots;
    if (const char* e = getenv("TFFT_COLS_DIRECT_MAX_LOG")) c->cols_direct_max_log = atoi(e);
    if (const char* e = getenv("TFFT_COLS_LOG_N1")) c->cols_force_log_n1 = atoi(e);
    c->n_cus = prop.multiProcessorCount;
    c->collect_resident = collect_bracket_resident_blocks();
    if (const char* e = getenv("TFFT_FUSE")) c->fuse = atoi(e);
    if (const char* e = getenv("TFFT_FUSE_WIDE")) c->fuse_wide = atoi(e);
    if (const char* e = getenv("TFFT_FUSE_LIVE")) c->fuse_live = atoi(e);
    if (const char* e = getenv("TFFT_EMBED_DELTA")) c->embed_delta = atoi(e);
    if (const char* e = getenv("TFFT_STATS_ASYNC")) c->stats_async = atoi(e);
    if (const char* e = getenv("TFFT_STATS_M2")) c->stats_m2 = atoi(e);
    if (const char* e = getenv("TFFT_STATS_SKEW")) c->stats_skew = atoi(e);
    if (const char* e = getenv("TFFT_STREAMS")) c->n_streams = atoi(e);
    if (const char* e = getenv("TFFT_TILE_READ")) c->tile_read = atoi(e);
    if (const char* e = getenv("TFFT_DC_BIAS")) c->dc_bias = (float)atof(e);
    if (const char* e = getenv("TFFT_MEDIAN_FALLBACK")) c->median_force_fallback = atoi(e);
    if (const char* e = getenv("TFFT_STATS_FUSED")) c->stats_fused = atoi(e);
    if (const char* e = getenv("TFFT_STATS_COMPACT")) c->stats_compact = atoi(e);
    if (const char* e = getenv("TFFT_GRAPHS")) c->graph_max_images = atoi(e);
    if (const char* e = getenv("TFFT_EXACT_STATS")) c->exact_stats = atoi(e);
    if (const char* e = getenv("TFFT_BATCH_EXACT_TRACE")) c->bx_trace = atoi(e);
    if (const char* e = getenv("TFFT_STATS_TILE")) c->stats_tile = atoi(e);
    if (const char* e = getenv("TFFT_EMBED_TILE_FUSE")) c->embed_tile_fuse = atoi(e);
    if (const char* e = getenv("TFFT_STATS_PRIO")) c->stats_prio = atoi(e);
    if (const char* e = getenv("TFFT_STATS_FAIL_ONCE")) c->stats_fail_once = atoi(e);
    if (const char* e = getenv("TFFT_STATS_TILE_STEP")) { c->stats_tile_step = atoi(e); if (c->stats_tile_step < 8) c->stats_tile_step = 8; c->stats_tile_step_forced = 1; }
    if (const char* e = getenv("TFFT_COLS_TILES")) { c->cols_tiles_per_block = atoi(e) > 0 ? atoi(e) : 1; c->cols_tiles_forced = 1; }
    if (const char* e = getenv("TFFT_COLS_TILES_EMBED")) c->cols_tiles_embed = atoi(e) > 0 ? atoi(e) : 0;
    if (const char* e = getenv("TFFT_COLS_TILES_STAT")) c->cols_tiles_stat = atoi(e) > 0 ? atoi(e) : 0;
    if (const char* e = getenv("TFFT_COLS_TILES_READ")) c->cols_tiles_read = atoi(e) > 0 ? atoi(e) : 1;
    if (c->cols_direct_max_log > 10) c->cols_direct_max_log = 10;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { delete c; return TFFT_E_HIP; }
    c->own_stream = true;
    (void)hipEventCreate(&c->ev_t0); (void)hipEventCreate(&c->ev_t1);
    c->slots.resize(n_slots);
    const size_t M = (size_t)pw / 2;
    c->slot_stride = 3 * (size_t)ph * M;
    // one slot per value of a plane (PH*(M+1)) + the slack of COLS_STAT's per-wave reservations (TFFT_STAT_RESV slots at a time: < 19 % even
    // when every value is a candidate)
    c->cand_stride = (size_t)ph * (M + 1) + (size_t)ph * M / 4 + 256;
    c->img_stride_b = (((size_t)max_w * max_h * 3 + 255) / 256) * 256;
    const size_t ns = (size_t)n_slots;
    int rc = dev_alloc(c, (void**)&c->img_pool, ns * c->img_stride_b + 256);
    if (!rc) rc = dev_alloc(c, (void**)&c->spec_pool, ns * c->slot_stride * sizeof(float2));
    if (!rc) rc = dev_alloc(c, (void**)&c->tmp_pool, ns * c->slot_stride * sizeof(float2));
    if (!rc) rc = dev_alloc(c, (void**)&c->cand_pool, ns * 3 * c->cand_stride * sizeof(unsigned));
    if (!rc) rc = dev_alloc(c, (void**)&c->col0_pool, ns * 3 * (size_t)ph * sizeof(float2));
    if (!rc) rc = dev_alloc(c, (void**)&c->sel, ns * 3 * sizeof(SelectState));
    if (!rc) rc = dev_alloc(c, (void**)&c->med, ns * 3 * sizeof(float));
    if (!rc) rc = dev_alloc(c, (void**)&c->partial, (ns * 3 * TFFT_STAT_MAX_BLOCKS + ns) * sizeof(unsigned));      // + one flag per image (batch capacity)
    if (!rc) rc = dev_alloc(c, (void**)&c->amb, ns * 3 * TFFT_AMB_CAP * sizeof(float));
    if (!rc) rc = dev_alloc(c, (void**)&c->usable, ns * sizeof(unsigned long long));
    if (!rc) rc = dev_alloc(c, (void**)&c->err, sizeof(int));
    if (!rc) rc = dev_alloc(c, (void**)&c->trash, 8192);
    if (!rc) rc = dev_alloc(c, (void**)&c->last_row, 2 * sizeof(int));
    if (!rc && hipMemset(c->err, 0, sizeof(int)) != hipSuccess) rc = TFFT_E_HIP;
    if (!rc && hipMemset(c->sel, 0, ns * 3 * sizeof(SelectState)) != hipSuccess) rc = TFFT_E_HIP;      // the compact statistics pipeline starts from clean histograms
    if (!rc && hipDeviceSynchronize() != hipSuccess) rc = TFFT_E_HIP;
    if (rc != TFFT_OK) { tfft_destroy(c); return rc; }
    *out = c;
    return TFFT_OK;
}

int tfft_destroy(tfft_ctx* c) {
    if (!c) return TFFT_OK;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    invalidate_graphs(c);
    (void)hipFree(c->img_pool); (void)hipFree(c->spec_pool); (void)hipFree(c->tmp_pool); (void)hipFree(c->cand_pool);
    (void)hipFree(c->col0_pool);
    (void)hipFree(c->sel); (void)hipFree(c->med); (void)hipFree(c->partial); (void)hipFree(c->amb); (void)hipFree(c->usable); (void)hipFree(c->err); (void)hipFree(c->ex_cand); (void)hipFree(c->ex_val); (void)hipFree(c->ex_below); (void)hipFree(c->ex_n); for (auto& kv : c->ex_table) (void)hipFree(kv.second); (void)hipFree(c->trash); (void)hipFree(c->bit_index); (void)hipFree(c->last_row); (void)hipFree(c->ph_jit);
    (void)hipFree(c->fit_d); (void)hipFree(c->fit_mu); (void)hipFree(c->fit_part); (void)hipFree(c->fit_cnt); (void)hipFree(c->fit_iters); (void)hipFree(c->fit_wrong);
    (void)hipFree(c->bx_win); (void)hipFree(c->bx_cand); (void)hipFree(c->bx_below); (void)hipFree(c->bx_n); (void)hipFree(c->bx_idx); (void)hipFree(c->bx_grp);
    (void)hipFree(c->bx_part); (void)hipFree(c->bx_val); (void)hipFree(c->an_buf);
    for (auto& b : c->tb) { (void)hipFree(b.cnt); (void)hipFree(b.off); (void)hipFree(b.ent); (void)hipFree(b.fl); (void)hipFree(b.pb); (void)hipFree(b.jp); }
    for (auto& kv : c->tw) (void)hipFree(kv.second);
    for (auto& kv : c->dc) (void)hipFree(kv.second);
    (void)hipFree(c->stage_bins); (void)hipFree(c->stage_bits); (void)hipFree(c->stage_jit); (void)hipFree(c->stage_out);
    (void)hipFree(c->out_pool); (void)hipFree(c->stream_bits); (void)hipFree(c->stream_plen);
    (void)hipFree(c->sio_hdr); (void)hipFree(c->sio_pay); (void)hipFree(c->sio_status);
    for (int i = 0; i < 4; i++) { if (c->ev_in[i]) (void)hipEventDestroy(c->ev_in[i]); if (c->ev_comp[i]) (void)hipEventDestroy(c->ev_comp[i]); if (c->ev_out[i]) (void)hipEventDestroy(c->ev_out[i]); }
    if (c->s_in) (void)hipStreamDestroy(c->s_in);
    if (c->stream2) (void)hipStreamDestroy(c->stream2);
    for (int i = 0; i < 2; i++) {
        if (c->stream_stats[i]) (void)hipStreamDestroy(c->stream_stats[i]);
        if (c->ev_stats_fork[i]) (void)hipEventDestroy(c->ev_stats_fork[i]);
        if (c->ev_stats_join[i]) (void)hipEventDestroy(c->ev_stats_join[i]);
    }
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    if (c->ev_join) (void)hipEventDestroy(c->ev_join);
    if (c->s_out) (void)hipStreamDestroy(c->s_out);
    if (c->ev_t0) (void)hipEventDestroy(c->ev_t0);
    if (c->ev_t1) (void)hipEventDestroy(c->ev_t1);
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return TFFT_OK;
}

int tfft_set_stream(tfft_ctx* c, void* hip_stream) {
    if (!c) return TFFT_E_INVALID;
    invalidate_graphs(c);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
    c->stream = (hipStream_t)hip_stream;
    c->own_stream = false;
    return TFFT_OK;
}

int tfft_sync(tfft_ctx* c) {
    if (!c) return TFFT_E_INVALID;
    return check_err_flag(c);
}

int tfft_last_hip_error(const tfft_ctx* c) { return c ? c->last_hip : 0; }

int tfft_plan_info(const tfft_ctx* c, int w, int h, int n_images, int info[4]) {
    if (!c || !info || w < 1 || h < 1 || n_images < 1) return TFFT_E_INVALID;
    int pw = next_pow2(w), ph = next_pow2(h);
    if (pw < 2) pw = 2;
    if (pw > TFFT_MAX_DIM || ph > TFFT_MAX_DIM) return TFFT_E_TOO_LARGE;
    const ColPlan p = plan_cols(c, ph, pw, n_images);
    info[0] = p.direct ? 1 : 0; info[1] = p.log_n1; info[2] = p.log_n2; info[3] = p.fused_fwd ? 1 : 0;
    return TFFT_OK;
}
size_t tfft_device_bytes(const tfft_ctx* c) { return c ? c->dev_bytes : 0; }

int tfft_forward_rgb8_dev(tfft_ctx* c, int slot, const void* rgb_dev, int w, int h, int center, int* pw, int* ph) {
    if (!slot_ok(c, slot) || !rgb_dev) return TFFT_E_INVALID;
    Slot& s = c->slots[slot];
    int rc = set_geometry(c, s, w, h, center);
    if (rc) return rc;
    if (pw) *pw = s.PW;
    if (ph) *ph = s.PH;
    rc = enqueue_forward(c, slot, 1, (const uint8_t*)rgb_dev, c->stream);
    s.rgb_src = (const uint8_t*)rgb_dev;
    return rc;
}

int tfft_forward_rgb8(tfft_ctx* c, int slot, const uint8_t* rgb, int w, int h, int center, int* pw, int* ph) {
    if (!slot_ok(c, slot) || !rgb) return TFFT_E_INVALID;
    Slot& s = c->slots[slot];
    int rc = set_geometry(c, s, w, h, center);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(c->img(slot), rgb, (size_t)w * h * 3, hipMemcpyHostToDevice, c->stream));
    if (pw) *pw = s.PW;
    if (ph) *ph = s.PH;
    rc = enqueue_forward(c, slot, 1, c->img(slot), c->stream);
    s.rgb_src = c->img(slot);
    return rc;
}

// ---- exact statistics of a single resident image (tfft_exact.hip): the bins whose fp32 magnitude lies within a window of the decision
// value are re-evaluated in fp64 from the pixels, everything else is counted on the fp32 spectrum
namespace {
constexpr int EX_CAP = 4096;          // candidate slots per plane
constexpr int EX_SPLIT = 64;          // workgroups (row ranges) a candidate's sum is dealt to, at most

int exact_buffers(tfft_ctx* c) {
    if (c->ex_cand) return TFFT_OK;
    if (dev_alloc(c, (void**)&c->ex_cand, (size_t)3 * EX_CAP * sizeof(ExactCand)) || dev_alloc(c, (void**)&c->ex_val, (size_t)3 * EX_CAP * EX_SPLIT * sizeof(double2)) ||
        dev_alloc(c, (void**)&c->ex_below, 3 * sizeof(unsigned long long)) || dev_alloc(c, (void**)&c->ex_n, 3 * sizeof(unsigned)))
        return TFFT_E_NOMEM;
    return TFFT_OK;
}
bool exact_possible(const tfft_ctx* c, const Slot& s) {
    return c->exact_stats && s.rgb_src && s.PW == s.PWi && s.PWi <= 8192 && s.PH <= 65535 && s.PWi <= 65535;
}
// exp(2 pi i j/PW) in fp64 (device), made once per width
int exact_table(tfft_ctx* c, int PW, const double2** out) {
    auto it = c->ex_table.find(PW);
    if (it != c->ex_table.end()) { *out = it->second; return TFFT_OK; }
    double2* t = nullptr;
    if (dev_alloc(c, (void**)&t, (size_t)PW * sizeof(double2))) return TFFT_E_NOMEM;
    HIPCHK(c, launch_exact_table(t, PW, c->stream));
    c->ex_table[PW] = t;
    *out = t;
    return TFFT_OK;
}
// the row bands a candidate's sum is dealt to: the single-image and the batched calls cut alike, hence add the same partials
int exact_split(int H) { return std::min(std::max(H / 32, 1), EX_SPLIT); }
// ---- the decision rules of the exact statistics, one copy for the single-image calls and the batched embeds (DESIGN.md section 11 promises
// that they agree).  A candidate: its fp64 magnitude (std::abs(complex<double>) of S:406 / S:1004), its fp32 |F|^2, the weight it carries
struct ExactPt { double mag; float m2; unsigned long long w; };
double exact_emax(const std::vector<ExactPt>& pt) {
    double emax = 0.0;
    for (const ExactPt& q : pt) emax = fmax(emax, fabs(q.mag - sqrt((double)q.m2)));
    return emax;      // the largest fp32 error seen on a window's own bins
}
// Median (median_abs, S:404-409) from the candidates of a window of relative half-width rel around the fp32 median m32 and the weight below
// it.  False (widen) unless the window holds the rank and is 4 x wider than the error seen on its own bins (else a bin outside could belong inside)
bool exact_median_rule(const std::vector<ExactPt>& pt, unsigned long long outside, unsigned long long rank, double rel, float m32, double* med) {
    unsigned long long wsum = 0;
    for (const ExactPt& q : pt) wsum += q.w;
    if (!(outside <= rank && rank < outside + wsum) || 4.0 * exact_emax(pt) > rel * (double)m32) return false;
    std::vector<size_t> ord(pt.size());
    for (size_t i = 0; i < ord.size(); i++) ord[i] = i;
    std::sort(ord.begin(), ord.end(), [&](size_t a, size_t b) { return pt[a].mag < pt[b].mag; });
    unsigned long long cum = outside;
    *med = (double)m32;
    for (size_t k = 0; k < ord.size(); k++) { cum += pt[ord[k]].w; if (rank < cum) { *med = pt[ord[k]].mag; break; } }
    return true;
}
// Count (S:998-1008) of one plane: the weight outside the window plus the candidates not below thr, halved; false (widen) as above
bool exact_count_rule(const std::vector<ExactPt>& pt, unsigned long long outside, double rel, double thr, unsigned long long* count) {
    unsigned long long cnt = outside;
    for (const ExactPt& q : pt)
        if (!(q.mag < thr)) cnt += q.w;          // S:1004: `if (std::abs(F) < thr) continue`
    if (4.0 * exact_emax(pt) > rel * thr) return false;
    *count = cnt / 2;                            // S:1007: c/2 per plane
    return true;
}
struct ExactOut { std::vector<ExactPt> pt[3]; unsigned long long outside[3]; };
// one collect + evaluate round with the fp32 |F|^2 windows [lo2, hi2] per plane; false in `ok` when a candidate list overflowed
int exact_round(tfft_ctx* c, int slot, const ExactCollect& P, ExactOut& o, bool& ok) {
    const Slot& s = c->slots[slot];
    int rc = exact_buffers(c);
    if (rc) return rc;
    HIPCHK(c, launch_exact_collect(c->spec(slot), P, c->ex_cand, c->ex_below, c->ex_n, c->stream));
    unsigned n[3];
    HIPCHK(c, hipMemcpyAsync(n, c->ex_n, sizeof n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(o.outside, c->ex_below, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    ok = n[0] <= (unsigned)EX_CAP && n[1] <= (unsigned)EX_CAP && n[2] <= (unsigned)EX_CAP;
    if (!ok) return TFFT_OK;
    const double2* table = nullptr;
    rc = exact_table(c, s.PWi, &table);
    if (rc) return rc;
    const int split = exact_split(s.H);
    for (int p = 0; p < 3; p++) {
        o.pt[p].resize(n[p]);
        if (!n[p]) continue;
        HIPCHK(c, launch_exact_eval(s.rgb_src, s.W, s.H, s.PWi, s.PH, s.center, c->ex_cand + (size_t)p * EX_CAP, n[p], split, table,
                                    c->ex_val + (size_t)p * EX_CAP * EX_SPLIT, c->stream));
    }
    std::vector<double2> v((size_t)EX_CAP * EX_SPLIT);
    std::vector<ExactCand> cand((size_t)EX_CAP);
    for (int p = 0; p < 3; p++) {
        if (!n[p]) continue;
        HIPCHK(c, hipMemcpyAsync(cand.data(), c->ex_cand + (size_t)p * EX_CAP, n[p] * sizeof(ExactCand), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(v.data(), c->ex_val + (size_t)p * EX_CAP * EX_SPLIT, (size_t)n[p] * split * sizeof(double2), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        for (unsigned i = 0; i < n[p]; i++) {
            double re = 0.0, im = 0.0;
            for (int k = 0; k < split; k++) { re += v[(size_t)i * split + k].x; im += v[(size_t)i * split + k].y; }      // fixed order: deterministic
            o.pt[p][i] = ExactPt{hypot(re, im), cand[i].m2, cand[i].w};
        }
    }
    return TFFT_OK;
}
// fp32 window around a decision value d (> 0) on |F|^2: relative half-width `rel`, rounded outwards
void exact_window(double d, double rel, float& lo2, float& hi2) {
    const double lo = d * (1.0 - rel), hi = d * (1.0 + rel);
    lo2 = nextafterf((float)(lo * lo), -INFINITY); hi2 = nextafterf((float)(hi * hi), INFINITY);
    if (!(lo2 > 0.f)) lo2 = 0.f;
}
// median_abs S:404-409 for the three planes, refined from the fp32 medians m32; false when the refinement did not apply
bool exact_medians(tfft_ctx* c, int slot, const float m32[3], double med[3], int* rc_out) {
    const Slot& s = c->slots[slot];
    *rc_out = TFFT_OK;
    c->ex_last[0] = c->ex_last[1] = c->ex_last[2] = 0;
    if (!exact_possible(c, s)) return false;
    const unsigned long long rank = ((unsigned long long)s.PH * s.PW) / 2;
    double rel = 2e-6;                   // ~16 sigma of the fp32 transform's error at the median's magnitude (measured 1.2e-7 relative)
    for (int attempt = 0; attempt < 5; attempt++, rel *= 4.0) {
        ExactCollect P{};
        P.PH = s.PH; P.PW = s.PWi; P.PW_full = s.PW; P.cap = 0; P.cap_cand = EX_CAP;
        for (int p = 0; p < 3; p++) exact_window((double)m32[p], rel, P.lo2[p], P.hi2[p]);
        ExactOut o; bool ok = false;
        int rc = exact_round(c, slot, P, o, ok);
        if (rc) { *rc_out = rc; return false; }
        if (!ok) return false;           // a flat spectrum (thousands of bins within 1e-6 of the median): keep the fp32 answer
        bool good = true;
        for (int p = 0; p < 3 && good; p++) {
            good = exact_median_rule(o.pt[p], o.outside[p], rank, rel, m32[p], &med[p]);
            if (good) c->ex_last[p] = (int)o.pt[p].size();
        }
        if (good) return true;
    }
    return false;
}
// Stream framing (S:986-995): a header byte becomes 24 stream bits (8 bits, each three times), a payload byte 56 (each seven times)
constexpr uint64_t kHeaderBytes = 38, kBitsPerHeaderByte = 24, kBitsPerPayloadByte = 56;
constexpr uint64_t kHeaderBits = kHeaderBytes * kBitsPerHeaderByte;      // 912
inline uint64_t stream_bits(uint64_t payload_len) { return kHeaderBits + payload_len * kBitsPerPayloadByte; }
// does the stream of a payload fit a walk of n_bins?  (Divides before it multiplies: a huge length must not wrap)
inline bool stream_fits(uint64_t n_bins, uint64_t payload_len) {
    return n_bins >= kHeaderBits && payload_len <= (n_bins - kHeaderBits) / kBitsPerPayloadByte;
}
// What a batched call hands each of its chunks: everything but the slots, the stream and the chunk's images and outputs.  The per-image
// arrays (device) are those of the chunk's first image; from(i) moves them on by i images and is the one place that states their strides.
struct ChunkArgs {
    const tfft_bin* bins = nullptr;      // one list of n_bits bins for every image (per_image: one list each)
    uint64_t n_bits = 0;
    double alpha = 0.0;
    double rmin = 0.0, rmax = 0.0, magmin = 0.0;      // the annulus and the threshold of the capacities (embeds)
    // the bit source of an embed: one byte per bit, n_bits per image -- or the packed frames of the stream pipelines (kHeaderBytes + plen
    // bytes per image), expanded by the kernels on the way: `limit` stream bits per image, the bin list may be longer
    const uint8_t* bits = nullptr;
    const uint8_t* hdr = nullptr; const uint8_t* pay = nullptr; uint64_t plen = 0, limit = ~0ull;
    // one walk per image (tfft_*_stream_batch_walks*, the fitted embed): `bins` are a chunk's g lists, image i's at bins + i*n_bits; jitter
    // (the same layout, or nullptr) and adaptive alpha come with them instead of from the context's phase options
    bool per_image = false; const float* jit = nullptr; bool adaptive = false;
    bool values_wanted = false;      // the caller reads the listed bins' values (the `fl` list) after the embed: the fitted embed
    static ChunkArgs list(const void* bins, uint64_t n_bits, double alpha) {
        ChunkArgs a;
        a.bins = (const tfft_bin*)bins; a.n_bits = n_bits; a.alpha = alpha;
        return a;
    }
    ChunkArgs& capacity(double lo, double hi, double mm) { rmin = lo; rmax = hi; magmin = mm; return *this; }
    ChunkArgs& plain(const void* b) { bits = (const uint8_t*)b; return *this; }
    ChunkArgs& frames(const void* h, const void* p, uint64_t len) {
        hdr = (const uint8_t*)h; pay = (const uint8_t*)p; plen = len; limit = stream_bits(len);      // S:986-995
        return *this;
    }
    ChunkArgs& walks(const void* j, int adapt) { per_image = true; jit = (const float*)j; adaptive = adapt != 0; return *this; }
    ChunkArgs& values() { values_wanted = true; return *this; }
    bool framed() const { return hdr != nullptr; }
    uint64_t stream_len() const { return limit < n_bits ? limit : n_bits; }      // the bits an image carries
    ChunkArgs from(size_t i) const {
        ChunkArgs a = *this;
        if (bits) a.bits += i * n_bits;
        if (hdr) a.hdr += i * kHeaderBytes;
        if (pay) a.pay += i * plen;
        if (per_image) { a.bins += i * n_bits; if (jit) a.jit += i * n_bits; }
        return a;
    }
};

// ---- exact capacities of the batched embeds (tfft_set_batch_exact).  A chunk's selected covers get a storing fp32
// forward into the slot spectra; then the single-image method (exact_medians, tfft_capacity) runs for all of them at once: one collect
// launch (per-image windows), one evaluate launch (k_exact_eval_batch: TFFT_EXACT_K candidates of an image plane per pass over its pixels),
// one in-order sum, one read per round.  The decisions are the single-image calls' own (exact_median_rule, exact_count_rule), the rounds
// and windows follow them; an image settles, widens or gives up on its own.
int bx_buffers(tfft_ctx* c) {
    if (c->bx_win) return TFFT_OK;
    const size_t n = (size_t)c->n_slots, nc = 3 * n * EX_CAP;
    if (dev_alloc(c, (void**)&c->bx_win, n * sizeof(ExactWin)) || dev_alloc(c, (void**)&c->bx_cand, nc * sizeof(ExactCandB)) ||
        dev_alloc(c, (void**)&c->bx_below, 3 * n * sizeof(unsigned long long)) || dev_alloc(c, (void**)&c->bx_n, 3 * n * sizeof(unsigned)) ||
        dev_alloc(c, (void**)&c->bx_idx, nc * sizeof(unsigned)) || dev_alloc(c, (void**)&c->bx_grp, nc * sizeof(ExactGroup)))
        return TFFT_E_NOMEM;
    return TFFT_OK;
}
// the partials and settled values of n dense candidates (grown on demand: a round rarely holds more than a few thousand, hence half again,
// not grown()).  Settling runs on the context's stream after the chunk's streams have joined and is never captured: no quiesce()
int bx_value_buffers(tfft_ctx* c, size_t n, int split) {
    const size_t np = n * (size_t)split;
    if (np > c->bx_part_cap) {
        (void)hipStreamSynchronize(c->stream);
        (void)hipFree(c->bx_part); c->bx_part = nullptr; c->bx_part_cap = 0;
        const size_t cap = np + np / 2 + 4096;
        if (dev_alloc(c, (void**)&c->bx_part, cap * sizeof(double2))) return TFFT_E_NOMEM;
        c->bx_part_cap = cap;
    }
    if (n > c->bx_val_cap) {
        (void)hipStreamSynchronize(c->stream);
        (void)hipFree(c->bx_val); c->bx_val = nullptr; c->bx_val_cap = 0;
        const size_t cap = n + n / 2 + 1024;
        if (dev_alloc(c, (void**)&c->bx_val, cap * sizeof(ExactVal))) return TFFT_E_NOMEM;
        c->bx_val_cap = cap;
    }
    return TFFT_OK;
}
// per (entry, plane) of a round: the candidates' settled values, the weight outside the window, whether the list fit
struct BxList { std::vector<ExactPt> v; unsigned long long outside = 0; bool ok = false; };
// one collect + evaluate round over the launch entries `win` (spectra at c->spec(s0) + img, covers at cov + img * img_bytes) -> out[3z + p]
int bx_round(tfft_ctx* c, int s0, const uint8_t* cov, size_t img_bytes, const ExactCollect& P, const std::vector<ExactWin>& win,
             std::vector<BxList>& out, unsigned* max_cand, hipStream_t st) {
    const Slot& s = c->slots[s0];
    const int nz = (int)win.size(), nl = 3 * nz;
    std::vector<unsigned> n((size_t)nl);
    std::vector<unsigned long long> below((size_t)nl);
    HIPCHK(c, hipMemcpyAsync(c->bx_win, win.data(), (size_t)nz * sizeof(ExactWin), hipMemcpyHostToDevice, st));
    HIPCHK(c, launch_exact_collect_batch(c->spec(s0), c->slot_stride, P, c->bx_win, nz, c->bx_cand, c->bx_below, c->bx_n, st));
    HIPCHK(c, hipMemcpyAsync(n.data(), c->bx_n, (size_t)nl * sizeof(unsigned), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(below.data(), c->bx_below, (size_t)nl * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    // dense candidates of the entries whose three lists fit, in list order; workgroups of up to TFFT_EXACT_K of one list
    std::vector<unsigned> idx;
    std::vector<ExactGroup> grp;
    out.assign((size_t)nl, BxList());
    for (int z = 0; z < nz; z++) {
        const bool fit = n[3 * z] <= (unsigned)EX_CAP && n[3 * z + 1] <= (unsigned)EX_CAP && n[3 * z + 2] <= (unsigned)EX_CAP;
        for (int p = 0; p < 3; p++) {
            const int l = 3 * z + p;
            out[l].ok = fit; out[l].outside = below[l];
            if (max_cand && n[l] > *max_cand) *max_cand = n[l];
            if (!fit) continue;
            for (unsigned k0 = 0; k0 < n[l]; k0 += TFFT_EXACT_K) {
                const unsigned cnt = n[l] - k0 < (unsigned)TFFT_EXACT_K ? n[l] - k0 : (unsigned)TFFT_EXACT_K;
                grp.push_back(ExactGroup{(unsigned)idx.size(), cnt});
                for (unsigned k = 0; k < cnt; k++) idx.push_back((unsigned)l * EX_CAP + k0 + k);
            }
        }
    }
    if (idx.empty()) return TFFT_OK;
    const double2* table = nullptr;
    int rc = exact_table(c, s.PWi, &table);
    if (rc) return rc;
    const int split = exact_split(s.H);
    rc = bx_value_buffers(c, idx.size(), split);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(c->bx_idx, idx.data(), idx.size() * sizeof(unsigned), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->bx_grp, grp.data(), grp.size() * sizeof(ExactGroup), hipMemcpyHostToDevice, st));
    HIPCHK(c, launch_exact_eval_batch(cov, img_bytes, s.W, s.H, s.PWi, s.PH, s.center, c->bx_cand, c->bx_idx, c->bx_grp, (unsigned)grp.size(), split,
                                      table, c->bx_part, st));
    HIPCHK(c, launch_exact_sum_batch(c->bx_part, split, c->bx_cand, c->bx_idx, (unsigned)idx.size(), c->bx_val, st));
    std::vector<ExactVal> v(idx.size());
    HIPCHK(c, hipMemcpyAsync(v.data(), c->bx_val, v.size() * sizeof(ExactVal), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    for (size_t i = 0; i < idx.size(); i++) out[idx[i] / EX_CAP].v.push_back(ExactPt{hypot(v[i].re, v[i].im), v[i].m2, v[i].w});
    return TFFT_OK;
}

// The chunk in slots [s0, s0+g): covers at cov (g images w*h*3 bytes apart, intact), fp32 medians in c->med, fp32 counts in `usable` (device).
// Settles the images the mode selects (NEAR: |count - L| <= guard) and overwrites their counts; state[i] = 1 / 0 / -1 (tfft_batch_exact_info).
// Synchronises st.
int bx_settle(tfft_ctx* c, int s0, int g, const uint8_t* cov, const ChunkArgs& a, unsigned long long* usable, int32_t* state, hipStream_t st) {
    const uint64_t L = a.stream_len();
    const double magmin = a.magmin;
    for (int i = 0; i < g; i++) state[i] = 0;
    if (!c->bx_mode || !usable || g <= 0) return TFFT_OK;
    int rc = bx_buffers(c);
    if (rc) return rc;
    const Slot& s = c->slots[s0];
    const size_t img_bytes = (size_t)s.W * s.H * 3;
    std::vector<unsigned long long> u((size_t)g);
    std::vector<float> m32((size_t)3 * g);
    HIPCHK(c, hipMemcpyAsync(u.data(), usable, (size_t)g * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(m32.data(), c->med + 3 * s0, (size_t)3 * g * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    std::vector<int> sel;
    for (int i = 0; i < g; i++) {
        const uint64_t d = u[i] >= L ? u[i] - L : L - u[i];
        if (c->bx_mode == TFFT_BATCH_EXACT_ALL || d <= c->bx_guard) sel.push_back(i);
    }
    if (sel.empty()) return TFFT_OK;
    for (int i : sel) state[i] = -1;
    Slot sx = s; sx.rgb_src = cov;                      // (exact_possible asks for an image to read)
    if (!exact_possible(c, sx)) return TFFT_OK;         // W < 2, PW > 8192, TFFT_EXACT_STATS=0: the fp32 counts stay
    const int n = (int)sel.size();
    // the selected covers packed to the front (NEAR): in the slots' image pool; a cover already there moves down only (j <= sel[j])
    const uint8_t* src = cov;
    if (n < g) {
        uint8_t* dst = c->img(s0);
        for (int j = 0; j < n; j++)
            if (cov + (size_t)sel[j] * img_bytes != dst + (size_t)j * img_bytes)
                HIPCHK(c, hipMemcpyAsync(dst + (size_t)j * img_bytes, cov + (size_t)sel[j] * img_bytes, img_bytes, hipMemcpyDeviceToDevice, st));
        src = dst;
    }
    rc = enqueue_forward(c, s0, n, src, st);            // the fp32 spectra the windows are taken on (one storing forward launch sequence)
    for (int j = 0; j < n; j++) { c->slots[s0 + j].has_spec = false; c->slots[s0 + j].rgb_src = nullptr; }
    if (rc) return rc;
    ExactCollect P{};
    P.PH = s.PH; P.PW = s.PWi; P.PW_full = s.PW; P.cap_cand = EX_CAP;
    unsigned max_cand = 0;
    int med_rounds = 0, cap_rounds = 0;
    // medians: rank PH*PW/2, window 2e-6 widened x4, at most 5 rounds (exact_medians)
    const unsigned long long rank = ((unsigned long long)s.PH * s.PW) / 2;
    std::vector<double> med((size_t)3 * n);
    std::vector<int> todo, done;
    for (int j = 0; j < n; j++) todo.push_back(j);
    double rel = 2e-6;
    for (int attempt = 0; attempt < 5 && !todo.empty(); attempt++, rel *= 4.0) {
        std::vector<ExactWin> win(todo.size());
        for (size_t z = 0; z < todo.size(); z++) {
            win[z].img = todo[z];
            for (int p = 0; p < 3; p++) exact_window((double)m32[3 * sel[todo[z]] + p], rel, win[z].lo2[p], win[z].hi2[p]);
        }
        P.cap = 0;
        std::vector<BxList> o;
        rc = bx_round(c, s0, src, img_bytes, P, win, o, &max_cand, st);
        if (rc) return rc;
        med_rounds++;
        std::vector<int> again;
        for (size_t z = 0; z < todo.size(); z++) {
            const int j = todo[z];
            if (!o[3 * z].ok) continue;                 // a flat spectrum: gives up (state -1), as the single-image call keeps its fp32 answer
            bool good = true;
            for (int p = 0; p < 3 && good; p++)
                good = exact_median_rule(o[3 * z + p].v, o[3 * z + p].outside, rank, rel, m32[3 * sel[j] + p], &med[3 * j + p]);
            if (good) done.push_back(j); else again.push_back(j);
        }
        todo.swap(again);
    }
    // capacities: thr = magmin * med, window 1e-3 widened x4, at most 4 rounds (tfft_capacity); a plane with thr <= 0 counts every annulus bin
    const CapParams cp = cap_params(c, s, a.rmin, a.rmax);
    P.cap = 1; P.s_lo = cp.s_lo; P.s_hi = cp.s_hi;
    std::vector<unsigned long long> exact_u(u);
    todo.clear();
    for (int j : done) {
        if (cp.bw > 0) todo.push_back(j);
        else { exact_u[sel[j]] = 0; state[sel[j]] = 1; }      // an empty annulus holds nothing
    }
    rel = 1e-3;
    for (int attempt = 0; attempt < 4 && !todo.empty(); attempt++, rel *= 4.0) {
        std::vector<ExactWin> win(todo.size());
        for (size_t z = 0; z < todo.size(); z++) {
            win[z].img = todo[z];
            for (int p = 0; p < 3; p++) {
                const double thr = magmin * med[3 * todo[z] + p];
                if (thr > 0.0) exact_window(thr, rel, win[z].lo2[p], win[z].hi2[p]);
                else win[z].lo2[p] = win[z].hi2[p] = -1.f;      // every |F|^2 lies above: the count is the annulus
            }
        }
        std::vector<BxList> o;
        rc = bx_round(c, s0, src, img_bytes, P, win, o, &max_cand, st);
        if (rc) return rc;
        cap_rounds++;
        std::vector<int> again;
        for (size_t z = 0; z < todo.size(); z++) {
            const int j = todo[z];
            if (!o[3 * z].ok) continue;
            bool good = true;
            unsigned long long total = 0;
            for (int p = 0; p < 3 && good; p++) {
                unsigned long long cnt = 0;
                good = exact_count_rule(o[3 * z + p].v, o[3 * z + p].outside, rel, magmin * med[3 * j + p], &cnt);
                total += cnt;
            }
            if (good) { exact_u[sel[j]] = total; state[sel[j]] = 1; }
            else again.push_back(j);
        }
        todo.swap(again);
    }
    if (c->bx_trace)
        fprintf(stderr, "tfft batch exact: %d of %d images settled, %d median + %d capacity rounds, max %u candidates per plane\n",
                (int)std::count(state, state + g, 1), g, med_rounds, cap_rounds, max_cand);
    HIPCHK(c, hipMemcpyAsync(usable, exact_u.data(), (size_t)g * sizeof(unsigned long long), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipStreamSynchronize(st));                 // (exact_u is a host array)
    return TFFT_OK;
}
// the state array of a batched embed call (nullptr without usable_out: the states of the last call that filled one stay)
int32_t* bx_begin(tfft_ctx* c, int n_images, const void* usable) {
    if (!usable || n_images < 0) return nullptr;
    c->bx_state.assign((size_t)n_images, 0);
    c->bx_last_n = n_images;
    return c->bx_state.data();
}
// the covers of a chunk whose embed writes over them (rgb_out overlaps rgb): copied to the slots' image pool first
const uint8_t* bx_keep_covers(tfft_ctx* c, int g, const uint8_t* rgb, const uint8_t* rgb_out, size_t img_bytes, hipStream_t st, int* rc) {
    *rc = TFFT_OK;
    const size_t len = (size_t)g * img_bytes;
    if (rgb_out + len <= rgb || rgb + len <= rgb_out) return rgb;
    if (hipMemcpyAsync(c->img(0), rgb, len, hipMemcpyDeviceToDevice, st) != hipSuccess) { *rc = TFFT_E_HIP; return rgb; }
    return c->img(0);
}
}  // namespace

int tfft_medians(tfft_ctx* c, int slot, double med[3]) {
    if (!slot_ok(c, slot) || !med) return TFFT_E_INVALID;
    if (!c->slots[slot].has_spec) return TFFT_E_STATE;
    int rc = enqueue_medians(c, slot, 1, c->stream);
    if (rc) return rc;
    float m[3];
    HIPCHK(c, hipMemcpyAsync(m, c->med + 3 * slot, sizeof m, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < 3; i++) med[i] = (double)m[i];
    // the fp32 medians locate the element; its value (and which of the near-equal neighbours it is) comes from fp64 sums over the pixels
    double ex[3];
    if (exact_medians(c, slot, m, ex, &rc)) { for (int i = 0; i < 3; i++) med[i] = ex[i]; }
    return rc;
}

int tfft_exact_info(const tfft_ctx* c, int n_fp64[3]) {
    if (!c || !n_fp64) return TFFT_E_INVALID;
    for (int i = 0; i < 3; i++) n_fp64[i] = c->ex_last[i];
    return TFFT_OK;
}

int tfft_median_path(tfft_ctx* c, int slot, int fast[3]) {
    if (!slot_ok(c, slot) || !fast) return TFFT_E_INVALID;
    SelectState* h = (SelectState*)malloc(3 * sizeof(SelectState));
    if (!h) return TFFT_E_NOMEM;
    hipError_t e = hipMemcpyAsync(h, c->sel + 3 * slot, 3 * sizeof(SelectState), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    for (int i = 0; i < 3; i++) fast[i] = (h[i].done == 1 && h[i].fast) ? 1 : 0;
    free(h);
    if (e != hipSuccess) { c->last_hip = (int)e; return TFFT_E_HIP; }
    return TFFT_OK;
}

int tfft_batch_medians(tfft_ctx* c, int slot, float med[3]) {
    if (!slot_ok(c, slot) || !med) return TFFT_E_INVALID;
    HIPCHK(c, hipMemcpyAsync(med, c->med + 3 * slot, 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return TFFT_OK;
}
int tfft_embed_plan_info(const tfft_ctx* c, int info[4]) {
    if (!c || !info) return TFFT_E_INVALID;
    for (int i = 0; i < 4; i++) info[i] = c->last_embed_path[i];
    return TFFT_OK;
}

int tfft_capacity(tfft_ctx* c, int slot, double rmin, double rmax, const double thr[3], uint64_t* usable) {
    if (!slot_ok(c, slot) || !thr || !usable) return TFFT_E_INVALID;
    Slot& s = c->slots[slot];
    if (!s.has_spec) return TFFT_E_STATE;
    CapParams p = cap_params(c, s, rmin, rmax);
    for (int i = 0; i < 3; i++) p.thr[i] = thr[i];
    // exact count (S:998-1008 on the reference's fp64 magnitudes): bins safely above the threshold are counted on the fp32 spectrum, the
    // few within a window of it are settled in fp64.  Small magnitudes carry the transform's ABSOLUTE error (~1e-7 of the spectrum's rms),
    // hence the wide relative window (1e-3) and the check against the error seen on the window's own bins.
    c->ex_last[0] = c->ex_last[1] = c->ex_last[2] = 0;
    if (exact_possible(c, s) && p.bw > 0 && thr[0] > 0.0 && thr[1] > 0.0 && thr[2] > 0.0) {
        double rel = 1e-3;
        for (int attempt = 0; attempt < 4; attempt++, rel *= 4.0) {
            ExactCollect P{};
            P.PH = s.PH; P.PW = s.PWi; P.PW_full = s.PW; P.cap = 1; P.cap_cand = EX_CAP; P.s_lo = p.s_lo; P.s_hi = p.s_hi;
            for (int q = 0; q < 3; q++) exact_window(thr[q], rel, P.lo2[q], P.hi2[q]);
            ExactOut o; bool ok = false;
            int rc = exact_round(c, slot, P, o, ok);
            if (rc) return rc;
            if (!ok) break;
            bool good = true;
            unsigned long long total = 0;
            for (int q = 0; q < 3 && good; q++) {
                unsigned long long cnt = 0;
                good = exact_count_rule(o.pt[q], o.outside[q], rel, thr[q], &cnt);
                total += cnt;
                c->ex_last[q] = (int)o.pt[q].size();
            }
            if (good) { *usable = total; return TFFT_OK; }
        }
        c->ex_last[0] = c->ex_last[1] = c->ex_last[2] = 0;
    }
    HIPCHK(c, launch_capacity(c->spec(slot), p, 1, nullptr, c->partial + (size_t)3 * slot * TFFT_STAT_MAX_BLOCKS,
                              c->usable + slot, c->stream, nullptr));
    unsigned long long u = 0;
    HIPCHK(c, hipMemcpyAsync(&u, c->usable + slot, sizeof u, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *usable = u;
    return TFFT_OK;
}

int tfft_lowfreq_mag(tfft_ctx* c, int slot, int region, double* out) {
    if (!slot_ok(c, slot) || !out || region < 1 || region > 8) return TFFT_E_INVALID;
    Slot& s = c->slots[slot];
    if (!s.has_spec || !s.rgb_src) return TFFT_E_STATE;
    if (region > s.PH || region > s.PW) return TFFT_E_INVALID;
    // fp64 inner products with the image itself (k_lowfreq_*_f64): scratch = tmp, free between forward and inverse
    const size_t row_bytes = (size_t)s.H * 3 * region * sizeof(double2), out_bytes = (size_t)3 * region * region * sizeof(double);
    if (row_bytes + out_bytes > c->slot_stride * sizeof(float2)) return TFFT_E_INVALID;
    double2* rowsum = (double2*)c->tmp(slot);
    double* d = (double*)((char*)rowsum + row_bytes);
    HIPCHK(c, launch_lowfreq_f64(s.rgb_src, s.W, s.H, s.PW, s.PH, s.center, region, rowsum, d, c->stream));
    HIPCHK(c, hipMemcpyAsync(out, d, out_bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return TFFT_OK;
}

int tfft_bins_register_dev(tfft_ctx* c, const void* bins_dev, uint64_t n) {
    if (!c) return TFFT_E_INVALID;
    invalidate_graphs(c);      // a captured sequence may have left the bucket build out
    for (auto& b : c->tb) { b.built_for = nullptr; b.row_for = nullptr; }
    c->reg_bins = (bins_dev && n) ? bins_dev : nullptr;
    c->reg_n = (bins_dev && n) ? n : 0;
    return TFFT_OK;
}

int tfft_set_bit_index(tfft_ctx* c, const uint32_t* bit_index, uint64_t n) {
    if (!c) return TFFT_E_INVALID;
    invalidate_graphs(c);
    for (auto& b : c->tb) { b.built_for = nullptr; b.row_for = nullptr; }
    if (!bit_index || n == 0) {            // back to "bins[i] carries bit i"
        HIPCHK(c, hipStreamSynchronize(c->stream));
        (void)hipFree(c->bit_index);
        c->bit_index = nullptr; c->bit_index_n = 0;
        return TFFT_OK;
    }
    if (n > 0xFFFFFFFFull) return TFFT_E_TOO_LARGE;
    // the kernels index bits/jitter/bits_out with these values: they must be a permutation of 0..n-1
    std::vector<uint64_t> seen((n + 63) / 64, 0);
    for (uint64_t i = 0; i < n; i++) {
        const uint32_t j = bit_index[i];
        if (j >= n || (seen[j >> 6] >> (j & 63)) & 1) return TFFT_E_INVALID;
        seen[j >> 6] |= 1ull << (j & 63);
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->bit_index_n != n || !c->bit_index) {
        (void)hipFree(c->bit_index);
        c->bit_index = nullptr; c->bit_index_n = 0;
        int rc = dev_alloc(c, (void**)&c->bit_index, n * sizeof(uint32_t));
        if (rc) return rc;
    }
    HIPCHK(c, hipMemcpy(c->bit_index, bit_index, n * sizeof(uint32_t), hipMemcpyHostToDevice));
    c->bit_index_n = n;
    return TFFT_OK;
}

int tfft_set_phase_options(tfft_ctx* c, const float* jitter, uint64_t n, int adaptive_alpha) {
    if (!c || (jitter && n == 0)) return TFFT_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    // calls enqueued before may still read the old array: it goes only once they are done
    int rc = quiesce(c);
    if (rc) return rc;
    c->ph_version++;
    c->ph_adaptive = adaptive_alpha ? 1 : 0;
    if (!jitter) {
        (void)hipFree(c->ph_jit);
        c->ph_jit = nullptr; c->ph_n = 0;
        return TFFT_OK;
    }
    if (c->ph_n != n || !c->ph_jit) {
        (void)hipFree(c->ph_jit);
        c->ph_jit = nullptr; c->ph_n = 0;
        rc = dev_alloc(c, (void**)&c->ph_jit, n * sizeof(float));
        if (rc) return rc;
    }
    HIPCHK(c, hipMemcpy(c->ph_jit, jitter, n * sizeof(float), hipMemcpyHostToDevice));
    c->ph_n = n;
    return TFFT_OK;
}

int tfft_set_batch_exact(tfft_ctx* c, int mode, uint64_t guard_bits) {
    if (!c || mode < TFFT_BATCH_EXACT_OFF || mode > TFFT_BATCH_EXACT_NEAR) return TFFT_E_INVALID;
    if (mode != TFFT_BATCH_EXACT_OFF) {
        HIPCHK(c, hipSetDevice(c->device));
        int rc = bx_buffers(c);
        if (rc) return rc;
    }
    c->bx_mode = mode; c->bx_guard = guard_bits;
    return TFFT_OK;
}

int tfft_batch_exact_info(const tfft_ctx* c, int n_images, int32_t* state_out) {
    if (!c || n_images < 0 || n_images > c->bx_last_n || (n_images && !state_out)) return TFFT_E_INVALID;
    for (int i = 0; i < n_images; i++) state_out[i] = c->bx_state[i];
    return TFFT_OK;
}

int tfft_embed_bins_dev(tfft_ctx* c, int slot, const void* bins, const void* bits, const void* jitter, uint64_t n,
                        double alpha, int adaptive, const double med[3]) {
    if (!slot_ok(c, slot) || (n && (!bins || !bits)) || (adaptive && !med)) return TFFT_E_INVALID;
    Slot& s = c->slots[slot];
    if (!s.has_spec || !index_ok(c, n)) return TFFT_E_STATE;
    EmbedParams p = embed_params(c, s, n, alpha, adaptive, med, jitter != nullptr);
    HIPCHK(c, launch_embed(c->spec(slot), (const tfft_bin*)bins, (const uint8_t*)bits, (const float*)jitter, p, 1, c->err, c->stream));
    return TFFT_OK;
}

int tfft_embed_bins(tfft_ctx* c, int slot, const tfft_bin* bins, const uint8_t* bits, const float* jitter, uint64_t n,
                    double alpha, int adaptive, const double med[3]) {
    if (!slot_ok(c, slot) || (n && (!bins || !bits))) return TFFT_E_INVALID;
    if (!c->slots[slot].has_spec) return TFFT_E_STATE;
    if (n == 0) return TFFT_OK;
    int rc = ensure_stage(c, n);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(c->stage_bins, bins, n * sizeof(tfft_bin), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->stage_bits, bits, n, hipMemcpyHostToDevice, c->stream));
    if (jitter) HIPCHK(c, hipMemcpyAsync(c->stage_jit, jitter, n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    rc = tfft_embed_bins_dev(c, slot, c->stage_bins, c->stage_bits, jitter ? c->stage_jit : nullptr, n, alpha, adaptive, med);
    if (rc) return rc;
    return check_err_flag(c);
}

int tfft_read_bins_dev(tfft_ctx* c, int slot, const void* bins, const void* jitter, uint64_t n, double alpha,
                       int adaptive, const double med[3], void* bits_out) {
    if (!slot_ok(c, slot) || (n && (!bins || !bits_out)) || (adaptive && !med)) return TFFT_E_INVALID;
    Slot& s = c->slots[slot];
    if (!s.has_spec || !index_ok(c, n)) return TFFT_E_STATE;
    EmbedParams p = embed_params(c, s, n, alpha, adaptive, med, jitter != nullptr);
    HIPCHK(c, launch_read(c->spec(slot), (const tfft_bin*)bins, (const float*)jitter, p, 1, (uint8_t*)bits_out, c->err, c->stream));
    return TFFT_OK;
}

int tfft_read_bins(tfft_ctx* c, int slot, const tfft_bin* bins, const float* jitter, uint64_t n, double alpha,
                   int adaptive, const double med[3], uint8_t* bits_out) {
    if (!slot_ok(c, slot) || (n && (!bins || !bits_out))) return TFFT_E_INVALID;
    if (!c->slots[slot].has_spec) return TFFT_E_STATE;
    if (n == 0) return TFFT_OK;
    int rc = ensure_stage(c, n);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(c->stage_bins, bins, n * sizeof(tfft_bin), hipMemcpyHostToDevice, c->stream));
    if (jitter) HIPCHK(c, hipMemcpyAsync(c->stage_jit, jitter, n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    rc = tfft_read_bins_dev(c, slot, c->stage_bins, jitter ? c->stage_jit : nullptr, n, alpha, adaptive, med, c->stage_out);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(bits_out, c->stage_out, n, hipMemcpyDeviceToHost, c->stream));
    return check_err_flag(c);
}

int tfft_inverse_rgb8_dev(tfft_ctx* c, int slot, void* rgb_out_dev) {
    if (!slot_ok(c, slot) || !rgb_out_dev) return TFFT_E_INVALID;
    if (!c->slots[slot].has_spec) return TFFT_E_STATE;
    return enqueue_inverse(c, slot, 1, (uint8_t*)rgb_out_dev, c->stream);
}

int tfft_inverse_rgb8(tfft_ctx* c, int slot, uint8_t* rgb_out) {
    if (!slot_ok(c, slot) || !rgb_out) return TFFT_E_INVALID;
    Slot& s = c->slots[slot];
    if (!s.has_spec) return TFFT_E_STATE;
    int rc = enqueue_inverse(c, slot, 1, c->img(slot), c->stream);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(rgb_out, c->img(slot), (size_t)s.W * s.H * 3, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return TFFT_OK;
}

int tfft_download_spectrum(tfft_ctx* c, int slot, float* out) {
    if (!slot_ok(c, slot) || !out) return TFFT_E_INVALID;
    Slot& s = c->slots[slot];
    if (!s.has_spec) return TFFT_E_STATE;
    const size_t n = (size_t)3 * s.PH * s.PW;
    float2* d = nullptr;
    if (hipMalloc((void**)&d, n * sizeof(float2)) != hipSuccess) return TFFT_E_NOMEM;
    hipError_t e = launch_export_full(c->spec(slot), s.PH, s.PWi, s.PW, d, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out, d, n * sizeof(float2), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(d);
    if (e != hipSuccess) { c->last_hip = (int)e; return TFFT_E_HIP; }
    return TFFT_OK;
}

// ---------------------------------------------------------------- batches
// Images are processed in chunks of n_slots; every stage of a chunk is ONE launch over all its
// images (grid.z = image), so each kernel sees thousands of workgroups.
static int batch_geometry(tfft_ctx* c, int g, int w, int h, int center) {
    for (int i = 0; i < g; i++) { int rc = set_geometry(c, c->slots[i], w, h, center); if (rc) return rc; }
    return TFFT_OK;
}

// the buckets of a bin list: one per (plane, row group of the last forward column step, 16-column tile) of an image like `s` in a launch of g
struct BucketGeom { int G, ntiles, nb; };
static BucketGeom bucket_geom(const tfft_ctx* c, const Slot& s, int g) {
    const ColPlan pl = plan_cols(c, s.PH, s.PWi, g);
    const int G = pl.direct ? 1 : (1 << pl.log_n1), ntiles = (s.PWi / 2 + 15) / 16;
    return BucketGeom{G, ntiles, 3 * ntiles * G};
}
// the head of a bucketed ColParams: the entries and offsets built on compute stream `which`
static ColParams bucketed_params(const tfft_ctx* c, int which) {
    ColParams cp{};
    cp.rd_bins = c->tb[which].ent; cp.rd_off = c->tb[which].off;
    return cp;
}

// device buffers of the tile buckets for `n` bins and `nb` buckets on compute stream `which`
static int ensure_buckets(tfft_ctx* c, int which, uint64_t n, int nb, bool with_values = false) {
    auto& b = c->tb[which];
    if (n > b.cap || !b.ent) {
        b.built_for = nullptr; b.cap = 0;
        const uint64_t cap = grown(n, 1024);
        const int rc = regrow(c, {{(void**)&b.ent, cap * sizeof(TileBin)}});
        if (rc) return rc;
        b.cap = cap;
    }
    if (nb + 1 > b.nb_cap || !b.cnt) {      // (sized exactly: the bucket count follows from the geometry, not from the list)
        b.built_for = nullptr; b.nb_cap = 0;
        const int rc = regrow(c, {{(void**)&b.cnt, (size_t)(nb + 1) * sizeof(unsigned)}, {(void**)&b.off, (size_t)(nb + 1 + (nb + 1023) / 1024) * sizeof(unsigned)}});
        if (rc) return rc;
        b.nb_cap = nb + 1;
    }
    if (with_values && (n * (uint64_t)c->n_slots > b.fl_cap || !b.fl)) {
        b.fl_cap = 0;
        const uint64_t cap = grown(n, 1024) * (uint64_t)c->n_slots;
        const int rc = regrow(c, {{(void**)&b.fl, cap * sizeof(float2)}, {(void**)&b.pb, cap}});
        if (rc) return rc;
        b.fl_cap = cap;
    }
    return TFFT_OK;
}

// the bins of a list bucketed by (plane, group, column tile) for the tile-resident read and the delta embedding; a registered list
// (tfft_bins_register_dev) keeps its buckets from one call to the next
static int build_buckets(tfft_ctx* c, int which, const tfft_bin* bins, uint64_t n_bits, const Slot& s, int G, hipStream_t st) {
    auto& tb = c->tb[which];
    const bool registered = bins == c->reg_bins && n_bits == c->reg_n;
    if (!(registered && tb.built_for == bins && tb.built_n == n_bits && tb.built_ph == s.PH && tb.built_pw == s.PWi && tb.built_g == G &&
          tb.built_index == c->bit_index)) {
        // a sequence captured for a registered list holds no bucket build: once the buffers describe another list it must not be replayed
        if (tb.built_for) c->graphs_stale = true;
        HIPCHK(c, launch_bucket_bins(bins, c->bit_index, n_bits, s.PH, s.PWi, G, tb.cnt, tb.off, tb.ent, c->err, c->tile_read == 2, st));
        tb.built_for = registered ? bins : nullptr; tb.built_n = n_bits; tb.built_ph = s.PH; tb.built_pw = s.PWi; tb.built_g = G; tb.built_index = c->bit_index;
        tb.built_bad = false;
        tb.jp_for = 0;
        if (registered && st == c->stream) {      // the cached buckets outlive this call: so does the verdict on the list (one sync per registration and geometry)
            const int rc = check_err_flag(c);
            if (rc == TFFT_E_BIN_RANGE) tb.built_bad = true;
            else if (rc) return rc;
        }
    }
    // every call on a registered list with bins outside the grid reports them (at its end, as the call that built the buckets does),
    // not only the first: the flag the builder raised is raised again
    if (tb.built_bad) HIPCHK(c, hipMemsetAsync(c->err, 0x01, sizeof(int), st));
    return TFFT_OK;
}

// room for n jitter phasors in bucket order on compute stream `which` (whatever was gathered there is gone when it grows)
static int ensure_jitter(tfft_ctx* c, int which, uint64_t n) {
    auto& tb = c->tb[which];
    if (n <= tb.jp_cap && tb.jp) return TFFT_OK;
    tb.jp_cap = 0; tb.jp_for = 0;
    const uint64_t cap = grown(n, 1024);
    int rc = regrow(c, {{(void**)&tb.jp, cap * sizeof(float2)}});
    if (rc) return rc;
    tb.jp_cap = cap;
    return TFFT_OK;
}

// the phase options' jitter in the order of the buckets just built (once per bucket build and setting: a registered list keeps it)
static int gather_jitter(tfft_ctx* c, int which, uint64_t n_bits, int nb, hipStream_t st) {
    auto& tb = c->tb[which];
    if (!c->ph_jit) return TFFT_OK;
    int rc = ensure_jitter(c, which, n_bits);
    if (rc) return rc;
    if (tb.jp_for != c->ph_version) {
        if (tb.jp_for) c->graphs_stale = true;      // (as for the buckets: a captured sequence without this gather must not be replayed)
        HIPCHK(c, launch_gather_jitter(tb.ent, tb.off + nb, c->ph_jit, n_bits, tb.jp, st));
        tb.jp_for = c->ph_version;
    }
    return TFFT_OK;
}

// the statistics' side stream: lowest priority, so that its small kernels fill gaps instead of taking workgroup slots from the transform
// they run beside (TFFT_STATS_PRIO=0: default priority)
static hipError_t create_stats_stream(tfft_ctx* c, hipStream_t* out) {
    int lo = 0, hi = 0;
    if (c->stats_prio && hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess && lo != hi)
        return hipStreamCreateWithPriority(out, hipStreamNonBlocking, lo);      // numerically greatest = lowest priority
    return hipStreamCreateWithFlags(out, hipStreamNonBlocking);
}

// the statistics' side stream of compute stream `which` (created on first use) forked off st ...
static int stats_fork(tfft_ctx* c, int which, hipStream_t st, hipStream_t* side) {
    if (!c->stream_stats[which]) {
        HIPCHK(c, create_stats_stream(c, &c->stream_stats[which]));
        HIPCHK(c, hipEventCreateWithFlags(&c->ev_stats_fork[which], hipEventDisableTiming));
        HIPCHK(c, hipEventCreateWithFlags(&c->ev_stats_join[which], hipEventDisableTiming));
    }
    HIPCHK(c, hipEventRecord(c->ev_stats_fork[which], st));
    HIPCHK(c, hipStreamWaitEvent(c->stream_stats[which], c->ev_stats_fork[which], 0));
    *side = c->stream_stats[which];
    return TFFT_OK;
}
// ... and joined back into it: whoever waits for st has the statistics too
static int stats_join(tfft_ctx* c, int which, hipStream_t st) {
    HIPCHK(c, hipEventRecord(c->ev_stats_join[which], c->stream_stats[which]));
    HIPCHK(c, hipStreamWaitEvent(st, c->ev_stats_join[which], 0));
    return TFFT_OK;
}

// Do the statistics of a batched delta embed run inside the last forward column step (COLS_STAT)?  Two-step column plans with 16 .. 512
// rows per step and whole column tiles; planes up to 2^24 bins (the compact select); an annulus that stays left of column PW/2
// (COLS_STAT counts stored bins only: on tall grids, whose annulus reaches the mirror half, the |F|^2 planes serve); launches of at
// least 2^24 bins -- four 1080p images, one 4K image (TFFT_STATS_TILE=2: any)
static bool tilestats_applies(const tfft_ctx* c, const Slot& s, const ColPlan& pl, const CapParams& p, int n) {
    if (!(c->stats_tile && c->stats_fused && c->stats_compact && !c->median_force_fallback)) return false;
    // a small launch is bound by its dependent launches: this form has 12, the planes' 7 (one 1080p image: 0.314 vs 0.283 ms per round trip)
    if (c->stats_tile < 2 && (unsigned long long)n * s.PH * s.PWi < (1ull << 24)) return false;
    const unsigned long long mirror_d = (unsigned long long)(p.PW - s.PWi / 2) * (unsigned long long)(p.PW - s.PWi / 2);
    return p.bw > 0 && p.s_lo <= p.s_hi && p.s_hi < 0xFFFFFFFFull && mirror_d > p.s_hi && !pl.direct && pl.log_n2 >= 4 && pl.log_n2 <= 9 &&
           (unsigned long long)s.PH * s.PWi <= TFFT_COMPACT_MAX_BINS && (s.PWi / 2) % 16 == 0;
}

// ... and does that step embed and run the first inverse column step on the same tile (COLS_STAT_EMBED)?  By default where the in-step
// statistics apply by their own size rule (a small launch forced into COLS_STAT by TFFT_STATS_TILE=2 keeps the pair); not with exact
// capacities on (their settle pass is kept on the sequence it was validated with).  L = 512 gains as L = 256 does (8 x 4K embed 2.47 ->
// 2.38 ms).  Not at L = 16, whatever the knob: with the DC term the fused form needs 220 registers where COLS_STAT needs
// 168 -- two workgroups per CU instead of three -- and nobody measured it; launch_cols has no such instantiation
static bool tile_fuse_applies(const tfft_ctx* c, const Slot& s, const ColPlan& pl, int n) {
    if (c->embed_tile_fuse <= 0 || c->bx_mode || pl.log_n2 < TFFT_TILE_FUSE_MIN_LOG) return false;
    return c->embed_tile_fuse >= 2 || (unsigned long long)n * s.PH * s.PWi >= (1ull << 24);
}

// The statistics after COLS_STAT, in two parts so that the first can run beside the inverse transform (embed_chunk):
//   select: the medians out of the staged candidates (5 small dependent launches, ~75 us of latency for a 32 x 1080p launch)
//   tail  : images with a plane the fast path could not settle get their spectrum after all -- the plain last forward step, gated (it
//           returns at once for the others) -- then the fallback kernels and the capacities.  Reads `tmp` (the last step's input):
//           the inverse in between keeps its intermediate in `spec` (StageMode::inv_via_spec)
static int enqueue_tilestats_select(tfft_ctx* c, int s0, int g, hipStream_t st) {
    const Slot& s = c->slots[s0];
    HIPCHK(c, launch_stat_select(s.PH, g, stat_bufs(c, s0, nullptr), st));
    return TFFT_OK;
}
static int enqueue_tilestats_tail(tfft_ctx* c, int s0, int g, const uint8_t* rgb_in, hipStream_t st, const CapParams& cap, unsigned long long* usable) {
    const Slot& s = c->slots[s0];
    const ColPlan pl = plan_cols(c, s.PH, s.PWi, g);
    ColParams gt{};
    gt.gate = c->sel + 3 * s0;
    StageMode mg; mg.fwd_mode = COLS_PLAIN; mg.fwd = &gt;
    int rc = enqueue_fft_stage(c, s0, g, pl.direct ? COLS_FWD_A : COLS_FWD_B, rgb_in, nullptr, st, mg);
    if (rc) return rc;
    HIPCHK(c, launch_stat_settle(c->spec(s0), s.PH, s.PWi, c->slot_stride, g, stat_bufs(c, s0, usable), stat_opts(c, &cap, false), st));
    for (int i = 0; i < g; i++) { c->slots[s0 + i].has_spec = false; c->slots[s0 + i].rgb_src = nullptr; }
    return TFFT_OK;
}

// forward transform + statistics of slots [s0, s0+g) without a stored spectrum (see ColParams::st_*): em carries the delta-embedding lists
// phases (tfft_profile_stage times them apart): 1 the steps before the last column step, 2 sample + bracket guess, 4 the COLS_STAT step,
// 8 select, 16 gated spectrum + fallbacks + capacity.  tile_fuse: the COLS_STAT step embeds and runs the first inverse step too (EmbedPath::tile_fuse)
static int enqueue_forward_tilestats(tfft_ctx* c, int s0, int g, const uint8_t* rgb_in, hipStream_t st, const ColParams& em, bool walks,
                                     const CapParams& cap, unsigned long long* usable, bool tile_fuse, int phases = 31) {
    const Slot& s = c->slots[s0];
    const ColPlan pl = plan_cols(c, s.PH, s.PWi, g);
    const int final_fwd = pl.direct ? COLS_FWD_A : COLS_FWD_B;
    // the sample: column tiles off, off + step, ..  -- centred in their strides (tiles 0, step, .. sit at the low-frequency end of every
    // stride and read a median several per cent too high: the bracket missed on every padded image)
    // eight sampled tiles per plane row group (every 8th of a 2048-wide grid's 64, every 16th of a 4096-wide one's 128): the sample pass is a
    // chain of dependent tile transforms per workgroup slot, its time goes with the tiles it walks (8 x 4K: 0.117 -> 0.0x ms)
    const int M = s.PWi / 2, ntiles = (M + 15) / 16;
    int step = c->stats_tile_step;
    while (!c->stats_tile_step_forced && ntiles / step > 8) step *= 2;
    // ... and of those tiles every 4th row group only, twice the tiles instead: a sixteenth of the plane rather than an eighth, spread over twice
    // the columns (the rows of a group are G apart: a regular subsample)
    const int G = 1 << pl.log_n1;
    int g_step = 1;
    if (!c->stats_tile_step_forced && G >= 8 && step >= 2 && ntiles / step >= 2) { g_step = 4; step /= 2; }
    const int off = ntiles > step / 2 ? step / 2 : 0;
    const int Ms = 16 * ((ntiles - off + step - 1) / step);
    int rc;
    for (int stage : {ROWS_FWD, COLS_FWD_A}) {
        if (stage == final_fwd || !(phases & 1)) break;
        rc = enqueue_fft_stage(c, s0, g, stage, rgb_in, nullptr, st);
        if (rc) return rc;
    }
    const StatBufs sb = stat_bufs(c, s0, usable);
    // (1) every step-th column tile, transformed and dropped into a histogram of |F|^2 (in LDS, ColParams::hist_sel): its median
    // brackets the plane's.  (First form: the tiles written side by side as a narrow spectrum + k_hist_spec over it -- 0.15 ms of a
    // 32 x 1080p launch where this takes 0.0x.)
    ColParams ex{};
    ex.tile_step = step; ex.tile_off = off; ex.out_M = Ms; ex.out_plane_stride = (size_t)s.PH * Ms; ex.out_img_stride = (size_t)3 * s.PH * Ms;
    ex.hist_sel = sb.st; ex.g_step = g_step; ex.g_off = g_step / 2;
    if (phases & 2) {
        StageMode ms;
        ms.fwd_mode = COLS_PLAIN; ms.fwd = &ex;
        rc = enqueue_fft_stage(c, s0, g, final_fwd, rgb_in, nullptr, st, ms);
        if (rc) return rc;
        HIPCHK(c, launch_stat_guess(nullptr, s.PH, s.PWi, Ms, ex.out_img_stride, 0, g, sb, stat_opts(c, &cap, false), st));
    }
    // (2) the last forward step: values of the listed bins + the bracket pass on every value
    if (phases & 4) {
        ColParams sp = em;
        sp.st_sel = sb.st; sp.st_cand = sb.cand; sp.st_cand_stride = sb.cand_stride; sp.st_partial = sb.partial; sp.st_amb = sb.amb; sp.st_col0 = sb.col0;
        sp.st_slo = cap.s_lo > 0xFFFFFFFFull ? 0xFFFFFFFFu : (unsigned)cap.s_lo; sp.st_shi = cap.s_hi > 0xFFFFFFFFull ? 0xFFFFFFFFu : (unsigned)cap.s_hi;
        sp.st_cap = 1; sp.st_PW = cap.PW;
        StageMode me; me.fwd_mode = tile_fuse ? COLS_STAT_EMBED : COLS_STAT; me.fwd = &sp; me.walks = walks;
        rc = enqueue_fft_stage(c, s0, g, final_fwd, rgb_in, nullptr, st, me);
        if (rc) return rc;
    }
    if (phases & 8) {
        rc = enqueue_tilestats_select(c, s0, g, st);
        if (rc) return rc;
    }
    if (phases & 16) return enqueue_tilestats_tail(c, s0, g, rgb_in, st, cap, usable);
    return TFFT_OK;
}

// the per-image lists of a chunk bucketed (launch_bucket_walks) on compute stream `which`: the shared-list buckets there are gone
static int build_buckets_walks(tfft_ctx* c, int which, const tfft_bin* bins, uint64_t n_bits, int g, const Slot& s, const BucketGeom& bg,
                               const float* jit, hipStream_t st) {
    const int G = bg.G;
    if ((uint64_t)g * n_bits > 0xFFFFFFFFull || (uint64_t)bg.nb * g + 1 > 1024ull * 1024ull) return TFFT_E_TOO_LARGE;
    int rc = ensure_buckets(c, which, (uint64_t)g * n_bits, bg.nb * g + 1);      // (+ the invalid bins' bucket)
    if (rc) return rc;
    auto& tb = c->tb[which];
    if (tb.built_for) c->graphs_stale = true;      // a sequence captured for a registered list left its bucket build out
    tb.built_for = nullptr; tb.jp_for = 0; tb.row_for = nullptr;
    HIPCHK(c, launch_bucket_walks(bins, n_bits, g, s.PH, s.PWi, G, tb.cnt, tb.off, tb.ent, c->err, st));
    if (!jit) return TFFT_OK;
    rc = ensure_jitter(c, which, (uint64_t)g * n_bits);
    if (rc) return rc;
    HIPCHK(c, launch_gather_jitter_walks(tb.ent, jit, n_bits, g, tb.jp, st));
    return TFFT_OK;
}
// ---- Which launch sequence a chunk takes.  Decided once, by the functions below, for the pipelines (embed_chunk, extract_chunk, fit_chunk)
// and for tfft_profile_stage alike: nobody else reads the knobs these look at (DESIGN.md section 4 has the table)
// the compute stream a chunk runs on: 0 the context's, 1 the one of the second half of a split chunk (TFFT_STREAMS=2)
static int stream_index(const tfft_ctx* c, hipStream_t st) { return (c->stream2 && st == c->stream2) ? 1 : 0; }
// adaptive alpha and jitter of a chunk: the per-image calls bring their own, the shared-list calls have the context's phase options
// (rc: the shared-list state does not mix with per-image walks)
struct PhaseOpts { int rc; bool adaptive; const float* jit; };
static PhaseOpts phase_opts(const tfft_ctx* c, const ChunkArgs& a) {
    if (!a.per_image) return PhaseOpts{TFFT_OK, c->ph_adaptive != 0, c->ph_jit};
    return PhaseOpts{(c->bit_index || c->ph_jit) ? TFFT_E_STATE : TFFT_OK, a.adaptive, a.jit};
}
// the statistics of an embed: none; the bracket pass inside the last forward step (COLS_STAT), then select chain and gated tail; medians +
// capacity in one sequence over the stored planes; medians, then the capacity as a pass of its own
enum StatsForm { STATS_NONE, STATS_IN_STEP, STATS_FUSED, STATS_SEPARATE };
// what the last forward column step leaves in `spec` (= ColParams::em_m2): the spectrum, |F|^2 planes + the packed column 0, nothing.  (A
// COLS_STAT step stores nothing and takes 0: the spectrum, where a plane needs it after all, comes from the gated plain step of the tail)
enum FwdStore { STORE_SPEC = 0, STORE_M2 = 1, STORE_NONE = 2 };
// delta: stego = cover + IFFT(F' - F) from the bucketed lists (else F' is written into the spectrum, k_embed, and inverted); side: the
// statistics run on the side stream, beside the inverse transform
// tile_fuse: the in-step statistics' launch is COLS_STAT_EMBED -- no COLS_EMBED launch, no values through the fl list
struct EmbedPath { bool delta; StatsForm stats; FwdStore store; bool side; bool tile_fuse; };
// stats: the chunk runs the statistics (capacities asked for, or adaptive alpha: see embed_chunk)
static EmbedPath embed_path(const tfft_ctx* c, const Slot& s, int g, const ChunkArgs& a, bool stats) {
    // (delta whatever the chunk size: the bytes of a stego image do not depend on how the batch was cut)
    EmbedPath p{c->embed_delta && a.alpha > 0.0 && a.alpha < M_PI && a.n_bits > 0, STATS_NONE, STORE_SPEC, false, false};
    if (!stats && p.delta && c->stats_m2) p.store = STORE_NONE;      // nobody reads the spectrum of a delta embed
    if (!stats) return p;
    const CapParams cap = cap_params(c, s, a.rmin, a.rmax);
    p.stats = (c->stats_fused && cap.bw > 0) ? STATS_FUSED : STATS_SEPARATE;
    if (!p.delta) return p;      // (the embed reads the medians' spectrum: everything in line)
    if (tilestats_applies(c, s, plan_cols(c, s.PH, s.PWi, g), cap, g)) p.stats = STATS_IN_STEP;
    else if (stats_m2_applies(c, s, cap)) p.store = STORE_M2;
    p.side = c->stats_async && !phase_opts(c, a).adaptive;      // (adaptive: the embed waits for the medians)
    p.tile_fuse = tile_fuse_applies(c, s, plan_cols(c, s.PH, s.PWi, g), g) && p.stats == STATS_IN_STEP && !phase_opts(c, a).adaptive && !a.values_wanted;
    return p;
}
// The spectrum is only ever read at the bins of the list.  READ_TILES: the bins bucketed by column tile, the last forward column step reads
// the bits out of its LDS-resident tiles -- no spectrum store, no k_read.  READ_ROWLIMIT: rows above the list's highest are not stored, then k_read
enum ReadForm { READ_TILES, READ_ROWLIMIT };
// (the bucket build is per call: it pays off from about 8 images per chunk; TFFT_TILE_READ=2/3 force it)
// registered: the list keeps its buckets (no per-call build to pay for): then the tile-resident read also serves small chunks of LARGE
// images (one 4K image: 0.739 -> 0.725 ms per round trip; one 1080p image has too few tiles to fill the chip: 0.265 -> 0.301)
// (an alpha outside (0, pi) takes the general phase comparison of k_read: the tile kernel reads the sign of Im only)
static ReadForm read_form(const tfft_ctx* c, const Slot& s, int g, const ChunkArgs& a, bool registered) {
    const bool reg_large = registered && (unsigned long long)s.PH * s.PWi >= (1ull << 23);
    const bool tiles = c->tile_read && a.n_bits > 0 && a.alpha > 0.0 && a.alpha < M_PI && (g >= 8 || c->tile_read >= 2 || reg_large);
    return tiles ? READ_TILES : READ_ROWLIMIT;
}

// Delta embedding.  The inverse transform is linear and IFFT(F) is the cover itself, so the stego image is cover + IFFT(F' - F),
// and F' - F is zero but for the bins of the list.  The bins are bucketed by column tile (the buckets extraction uses); the last
// forward column step, which has every tile in LDS, writes the values of the listed bins out in bucket order; the first inverse
// column step builds its tiles from that list instead of reading the spectrum; nothing writes F' anywhere, and the row kernel adds
// its result to the cover's pixels.  (The bucket build is per call unless the list is registered, tfft_bins_register_dev.)
// (jitter and adaptive alpha ride along: the entries carry the jitter phasor and the image's medians scale alpha)
// One sequence for every path: lists, forward, fork, statistics, embed + inverse, join, the in-kernel statistics' tail
static int embed_chunk_impl(tfft_ctx* c, int s0, int g, hipStream_t st, const ChunkArgs& a, const uint8_t* rgb_in, unsigned long long* usable,
                            uint8_t* rgb_out) {
    const Slot& s = c->slots[s0];
    const uint64_t n_bits = a.n_bits;
    const bool walks = a.per_image;
    if (!index_ok(c, n_bits) || !phase_ok(c, n_bits)) return TFFT_E_STATE;
    const PhaseOpts ph = phase_opts(c, a);
    if (ph.rc) return ph.rc;
    const EmbedPath path = embed_path(c, s, g, a, usable != nullptr);
    const bool in_step = path.stats == STATS_IN_STEP;
    c->last_embed_path[0] = path.delta; c->last_embed_path[1] = (int)path.stats; c->last_embed_path[2] = path.tile_fuse; c->last_embed_path[3] = path.side;
    EmbedParams ep = embed_params(c, s, n_bits, a.alpha, ph.adaptive, nullptr, ph.jit != nullptr);
    if (walks) ep.bins_stride = n_bits;
    if (ph.adaptive) ep.med_dev = c->med + 3 * s0;      // (the statistics below run before the embed: see EmbedPath::side)
    if (a.limit < n_bits) ep.limit = a.limit;      // the stream is shorter than the bin list (image i's bits still n_bits apart)
    if (a.framed()) { ep.frame_hdr = a.hdr; ep.frame_pay = a.pay; ep.frame_plen = a.plen; }
    CapParams cap = cap_params(c, s, a.rmin, a.rmax);
    cap.magmin = a.magmin;
    const int which = stream_index(c, st);
    ColParams em{};
    int rc;
    if (path.delta) {      // the lists of the chunk in bucket order
        const BucketGeom bg = bucket_geom(c, s, g);
        rc = ensure_buckets(c, which, n_bits, bg.nb, true);
        if (rc) return rc;
        rc = walks ? build_buckets_walks(c, which, a.bins, n_bits, g, s, bg, ph.jit, st) : build_buckets(c, which, a.bins, n_bits, s, bg.G, st);
        if (rc) return rc;
        auto& tb = c->tb[which];
        em = bucketed_params(c, which);
        em.em_fl = tb.fl + (size_t)s0 * n_bits; em.em_pb = tb.pb + (size_t)s0 * n_bits;
        em.em_n = walks ? 0 : n_bits; em.em_cos = ep.cos_a; em.em_sin = ep.sin_a;      // (walks: entry indices are absolute)
        if (!walks) rc = gather_jitter(c, which, n_bits, bg.nb, st);
        if (rc) return rc;
        em.em_jp = ph.jit ? tb.jp : nullptr;
        em.em_med = ph.adaptive ? c->med + 3 * s0 : nullptr; em.em_alpha = (float)a.alpha;
        em.em_m2 = path.store;
        if (path.store != STORE_SPEC) em.st_col0 = stat_col0(c, s0);
        // the stream bits in bucket order (the packed frames of the stream pipelines are expanded on the way).  (On the side stream
        // beside the forward transform it gained nothing measurable: 0.03 ms of 3.3.)
        if (walks) HIPCHK(c, launch_gather_bits_walks(tb.ent, a.bits, ep.frame_hdr, ep.frame_pay, ep.frame_plen, n_bits, ep.limit, g, tb.pb + (size_t)s0 * n_bits, st));
        else HIPCHK(c, launch_gather_bits(tb.ent, tb.off + bg.nb, a.bits, ep.frame_hdr, ep.frame_pay, ep.frame_plen, n_bits, ep.limit, g, tb.pb + (size_t)s0 * n_bits, st));
    }
    // forward.  In-kernel statistics: the sample, the bracket guess and the COLS_STAT step; neither the spectrum nor |F|^2 is stored (unless
    // a plane's bracket turns out wrong: then the gated plain step of the tail produces the spectrum for the fallback kernels)
    StageMode md;
    if (path.delta) { md.fwd_mode = COLS_EMIT; md.fwd = &em; md.walks = walks; }
    rc = in_step ? enqueue_forward_tilestats(c, s0, g, rgb_in, st, em, walks, cap, usable, path.tile_fuse, 7) : enqueue_forward(c, s0, g, rgb_in, st, md);
    if (rc) return rc;
    // the statistics.  With delta embedding nothing downstream reads them unless alpha is adaptive: on a side stream beside the inverse
    // transform, which does not wait for them (the in-kernel form's select chain is five small dependent launches)
    hipStream_t sst = st;
    if (path.side) { rc = stats_fork(c, which, st, &sst); if (rc) return rc; }
    switch (path.stats) {
        case STATS_NONE: break;
        case STATS_IN_STEP:
            rc = enqueue_tilestats_select(c, s0, g, sst);
            // adaptive: the embed needs the medians -- select, gated re-run and fallbacks all finish before the inverse step
            if (!rc && ph.adaptive) rc = enqueue_tilestats_tail(c, s0, g, rgb_in, st, cap, usable);
            break;
        case STATS_FUSED:      // S:922-923, S:998-1012 on the device, no host round trip: capacity is counted inside the median's full pass
            rc = enqueue_medians(c, s0, g, sst, &cap, usable, path.store == STORE_M2);
            break;
        case STATS_SEPARATE:
            rc = enqueue_medians(c, s0, g, sst);
            if (rc) return rc;
            HIPCHK(c, launch_capacity(c->spec(s0), cap, g, c->med + 3 * s0, stat_partial(c, s0), usable, sst, nullptr));
            break;
    }
    if (rc) return rc;
    if (!path.delta) {
        HIPCHK(c, launch_embed(c->spec(s0), a.bins, a.bits, ph.jit, ep, g, c->err, st));
        return enqueue_inverse(c, s0, g, rgb_out, st);
    }
    StageMode mi;
    mi.inv_mode = COLS_EMBED; mi.inv = &em; mi.walks = walks; mi.inv_cover = rgb_in; mi.inv_via_spec = in_step;
    mi.inv_first_done = path.tile_fuse;
    rc = enqueue_inverse(c, s0, g, rgb_out, st, mi);
    if (path.side) {            // (also after a failed inverse.)  Whoever waits for the context's stream has the capacities too
        const int rj = stats_join(c, which, st);
        if (rj) return rj;
    }
    if (rc || !in_step || ph.adaptive) return rc;
    return enqueue_tilestats_tail(c, s0, g, rgb_in, st, cap, usable);
}
// one chunk of an embed: the images rgb_in (g of them, packed) through slots [s0, s0+g) on stream st -> rgb_out, capacities -> usable (or nullptr)
static int embed_chunk(tfft_ctx* c, int s0, int g, hipStream_t st, const ChunkArgs& a, const uint8_t* rgb_in, unsigned long long* usable,
                       uint8_t* rgb_out) {
    // adaptive alpha needs every image's medians before the embed: the statistics run whether or not the caller asked for the
    // capacities (these then land in the context's own buffer)
    if (!usable && phase_opts(c, a).adaptive && a.n_bits > 0) usable = c->usable + s0;
    int rc = usable ? stats_clean_if_dirty(c, st) : TFFT_OK;
    if (!rc) rc = embed_chunk_impl(c, s0, g, st, a, rgb_in, usable, rgb_out);
    if (!rc && usable && c->stats_fail_once) {      // test hook (TFFT_STATS_FAIL_ONCE): as if the sequence had broken off -- garbage in the select state, an error out
        c->stats_fail_once = 0;
        HIPCHK(c, hipMemsetAsync(c->sel, 0x01, (size_t)c->n_slots * 3 * sizeof(SelectState), st));
        rc = TFFT_E_HIP;
    }
    if (rc && usable) c->stats_dirty = true;      // (the statistics may have been cut off between two of their launches)
    return rc;
}
// one chunk of an extract: the images rgb_in (g of them, packed) through slots [s0, s0+g) on stream st -> bits_out, n_bits per image
static int extract_chunk(tfft_ctx* c, int s0, int g, hipStream_t st, const ChunkArgs& a, const uint8_t* rgb_in, uint8_t* bits_out) {
    const Slot& s = c->slots[s0];
    const tfft_bin* bins = a.bins;
    const uint64_t n_bits = a.n_bits;
    const bool walks = a.per_image;
    if (!index_ok(c, n_bits) || !phase_ok(c, n_bits)) return TFFT_E_STATE;
    const PhaseOpts ph = phase_opts(c, a);
    if (ph.rc) return ph.rc;
    // adaptive alpha with |alpha| < pi/2: a = alpha*clamp(.., 0.5, 2) keeps the sign of alpha and |a| < pi, so the targets j +- a are
    // symmetric about j and j + pi and the bit is the side of that line -- what the fixed-alpha read decides.
    // Beyond, the decision depends on the medians: the single-image calls cover that case
    if (ph.adaptive && !(fabs(a.alpha) < M_PI / 2)) return TFFT_E_INVALID;
    const int which = stream_index(c, st);
    const bool registered = !walks && bins == c->reg_bins && n_bits == c->reg_n;
    auto& tb = c->tb[which];
    int rc;
    switch (read_form(c, s, g, a, registered)) {
        case READ_TILES: {
            const BucketGeom bg = bucket_geom(c, s, g);
            rc = walks ? TFFT_OK : ensure_buckets(c, which, n_bits, bg.nb);
            if (rc) return rc;
            HIPCHK(c, hipMemsetAsync(bits_out, 0, (size_t)g * n_bits, st));          // bins the walk would never produce read as 0 (k_read does the same)
            rc = walks ? build_buckets_walks(c, which, bins, n_bits, g, s, bg, ph.jit, st) : build_buckets(c, which, bins, n_bits, s, bg.G, st);
            if (rc) return rc;
            if (!walks) rc = gather_jitter(c, which, n_bits, bg.nb, st);
            if (rc) return rc;
            ColParams rd = bucketed_params(c, which);
            rd.rd_bits = bits_out; rd.rd_n = n_bits;
            rd.em_jp = ph.jit ? tb.jp : nullptr;
            StageMode md;
            md.fwd_mode = COLS_READ; md.fwd = &rd; md.walks = walks;
            rc = enqueue_forward(c, s0, g, rgb_in, st, md);
            if (rc) return rc;
            break;
        }
        case READ_ROWLIMIT: {
            int* last_row = c->last_row + which;
            if (!(registered && tb.row_for == bins && tb.row_n == n_bits && tb.row_ph == s.PH && tb.row_pw == s.PWi)) {
                // (one walk per image: the highest row over all the chunk's lists)
                HIPCHK(c, launch_bins_last_row(bins, walks ? (uint64_t)g * n_bits : n_bits, s.PH, s.PWi, last_row, st));
                tb.row_for = registered ? bins : nullptr; tb.row_n = n_bits; tb.row_ph = s.PH; tb.row_pw = s.PWi;
            }
            ColParams rl{};
            rl.last_row_dev = last_row;
            StageMode md;
            md.fwd_mode = COLS_ROWLIMIT; md.fwd = &rl;
            rc = enqueue_forward(c, s0, g, rgb_in, st, md);
            if (rc) return rc;
            EmbedParams ep = embed_params(c, s, n_bits, a.alpha, 0, nullptr, ph.jit != nullptr);
            if (walks) ep.bins_stride = n_bits;
            HIPCHK(c, launch_read(c->spec(s0), bins, ph.jit, ep, g, bits_out, c->err, st));
            break;
        }
    }
    for (int i = 0; i < g; i++) c->slots[s0 + i].has_spec = false;      // partial or no spectrum: not for tfft_medians & co
    return TFFT_OK;
}

// TFFT_STREAMS=2: a chunk of >= 8 images is split in two halves that run on two HIP streams, so that the
// latency-bound kernels of one half overlap the bandwidth-bound kernels of the other.  Returns the size of
// the first half (0: no split) after forking stream2 off the context stream.
static int split_fork(tfft_ctx* c, int g, int* h1) {
    *h1 = 0;
    if (c->n_streams < 2 || g < 8) return TFFT_OK;
    if (!c->stream2) {
        HIPCHK(c, hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking));
        HIPCHK(c, hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
        HIPCHK(c, hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming));
    }
    HIPCHK(c, hipEventRecord(c->ev_fork, c->stream));
    HIPCHK(c, hipStreamWaitEvent(c->stream2, c->ev_fork, 0));
    *h1 = g / 2;
    return TFFT_OK;
}
static int split_join(tfft_ctx* c) {
    HIPCHK(c, hipEventRecord(c->ev_join, c->stream2));
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_join, 0));
    return TFFT_OK;
}

}  // extern "C"
namespace {
// The slots and the stream of one chunk body: g images, the first of them image i1 of the call, in slots [s0, s0+g) on stream st
struct Chunk { int i1, s0, g; hipStream_t st; };
// The device arrays of an embed call.  With bx, the call's state array (bx_begin), the driver keeps the covers (rgb, which rgb_out may
// overlap) before a chunk and settles its capacities (usable) after it (tfft_set_batch_exact); nullptr for a call that does not settle
struct EmbedDev { const ChunkArgs& a; const uint8_t* rgb; uint8_t* rgb_out; unsigned long long* usable; int32_t* bx; };
// image i's entry of a per-image array (nullptr stays nullptr); strides: images w*h*3, headers kHeaderBytes, payloads their length, raw bits n_bins
template <class T> inline T* nth(T* base, size_t i, size_t stride = 1) { return base ? base + i * stride : nullptr; }
inline size_t image_bytes(int w, int h) { return (size_t)w * h * 3; }
// The chunk driver of the device-buffer batch calls: n_slots images at a time get their geometry, then body(Chunk) enqueues them.  split:
// under TFFT_STREAMS=2 a chunk of >= 8 images goes to the body as two halves on two streams.  The plain and the walks calls split; the shared-
// list stream pair must not: its extract indexes c->stream_bits and c->stream_plen without a slot offset (the halves would share the bits)
template <class Body>
int for_chunks(tfft_ctx* c, int n_images, int w, int h, int center, bool split, const EmbedDev* settle, Body&& body) {
    const size_t img_bytes = image_bytes(w, h);
    const bool settles = settle && settle->bx;
    for (int i0 = 0; i0 < n_images; i0 += c->n_slots) {
        const int g = (n_images - i0 < c->n_slots) ? n_images - i0 : c->n_slots;
        int rc = batch_geometry(c, g, w, h, center);
        if (rc) return rc;
        const uint8_t* cov = settles ? nth(settle->rgb, i0, img_bytes) : nullptr;
        if (settles && c->bx_mode) { cov = bx_keep_covers(c, g, cov, nth(settle->rgb_out, i0, img_bytes), img_bytes, c->stream, &rc); if (rc) return rc; }
        int h1 = 0;
        if (split) { rc = split_fork(c, g, &h1); if (rc) return rc; }
        for (int part = 0; part < (h1 ? 2 : 1); part++) {
            const int s0 = part ? h1 : 0, gp = h1 ? (part ? g - h1 : h1) : g;
            rc = body(Chunk{i0 + s0, s0, gp, part ? c->stream2 : c->stream});
            if (rc) return rc;
        }
        if (h1) { rc = split_join(c); if (rc) return rc; }
        if (settles) { rc = bx_settle(c, 0, g, cov, settle->a, settle->usable + i0, settle->bx + i0, c->stream); if (rc) return rc; }
    }
    return TFFT_OK;
}
// The chunk loop of the calls that need no more from a driver: at most `limit` images at a time, body(i0, g) for the images [i0, i0+g)
template <class Body>
int for_images(int n_images, int limit, Body&& body) {
    for (int i0 = 0; i0 < n_images; i0 += limit) {
        const int rc = body(i0, (n_images - i0 < limit) ? n_images - i0 : limit);
        if (rc) return rc;
    }
    return TFFT_OK;
}
// One per-image array of a host-buffer call: image i at host + i*stride bytes, a chunk's share staged at dev.  host == nullptr: the call
// does not use the array (a stride of 0 bytes: nothing to move)
struct HostArray { const void* host; void* dev; size_t stride; };
// the shares of the images [i0, i0+g) go up, in the order listed ...
int upload(tfft_ctx* c, const std::vector<HostArray>& arrays, int i0, int g, hipStream_t st) {
    for (const HostArray& a : arrays)
        if (a.host && a.stride) HIPCHK(c, hipMemcpyAsync(a.dev, (const char*)a.host + (size_t)i0 * a.stride, (size_t)g * a.stride, hipMemcpyHostToDevice, st));
    return TFFT_OK;
}
// ... and come down (the arrays listed here are the call's outputs: host is writable), then the stream is drained: the staging is free again
int download_sync(tfft_ctx* c, const std::vector<HostArray>& arrays, int i0, int g, hipStream_t st) {
    for (const HostArray& a : arrays)
        if (a.host && a.stride) HIPCHK(c, hipMemcpyAsync((char*)const_cast<void*>(a.host) + (size_t)i0 * a.stride, a.dev, (size_t)g * a.stride, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    return TFFT_OK;
}
// slots [0, g) lose their images: no spectrum, and no device image that tfft_lowfreq_mag could read again
void drop_images(tfft_ctx* c, int g) { for (int i = 0; i < g; i++) { c->slots[i].has_spec = false; c->slots[i].rgb_src = nullptr; } }
// the three device-buffer embeds: every chunk through embed_chunk
int embed_chunks(tfft_ctx* c, int n_images, int w, int h, int center, bool split, const EmbedDev& e) {
    const size_t img_bytes = image_bytes(w, h);
    return for_chunks(c, n_images, w, h, center, split, &e, [&](const Chunk& k) {
        return embed_chunk(c, k.s0, k.g, k.st, e.a.from(k.i1), nth(e.rgb, k.i1, img_bytes), nth(e.usable, k.i1), nth(e.rgb_out, k.i1, img_bytes));
    });
}
}  // namespace
extern "C" {

// host-side state a batch call leaves behind (what a graph replay has to redo): geometry set, no spectrum in any slot
static int batch_after(tfft_ctx* c, int n_images, int w, int h, int center) {
    const int g = n_images < c->n_slots ? n_images : c->n_slots;
    int rc = batch_geometry(c, g, w, h, center);
    if (rc) return rc;
    drop_images(c, g);
    return TFFT_OK;
}

int tfft_embed_batch_dev(tfft_ctx* c, int n_images, const void* rgb_dev, int w, int h, int center, const void* bins_dev,
                         const void* bits_dev, uint64_t n_bits, double alpha, double rmin, double rmax, double magmin,
                         void* usable_out_dev, void* rgb_out_dev) {
    if (!c || n_images < 0 || !rgb_dev || !rgb_out_dev || (n_bits && (!bins_dev || !bits_dev))) return TFFT_E_INVALID;
    if (!index_ok(c, n_bits) || !phase_ok(c, n_bits)) return TFFT_E_STATE;
    const ChunkArgs a = ChunkArgs::list(bins_dev, n_bits, alpha).capacity(rmin, rmax, magmin).plain(bits_dev);
    EmbedDev e{a, (const uint8_t*)rgb_dev, (uint8_t*)rgb_out_dev, (unsigned long long*)usable_out_dev, bx_begin(c, n_images, usable_out_dev)};
    if (e.bx && c->bx_mode) return embed_chunks(c, n_images, w, h, center, true, e);      // (settling synchronises: never captured or replayed)
    e.bx = nullptr;
    std::vector<uint64_t> key = {1, (uint64_t)n_images, key_bits(rgb_dev), (uint64_t)w, (uint64_t)h, (uint64_t)center, key_bits(bins_dev), key_bits(bits_dev),
                                       n_bits, key_bits(alpha), key_bits(rmin), key_bits(rmax), key_bits(magmin), key_bits(usable_out_dev),
                                       key_bits(rgb_out_dev), key_bits(c->bit_index), key_bits((double)c->dc_bias)};
    phase_key(c, key);
    return with_graph(c, n_images, key, [&] { return embed_chunks(c, n_images, w, h, center, true, e); },
                      [&] { return batch_after(c, n_images, w, h, center); });
}

// the generic read path stages its parameter block with a host -> device copy per call: not captured
static bool read_is_simple(double alpha) { return alpha > 0.0 && alpha < M_PI; }

int tfft_extract_batch_dev(tfft_ctx* c, int n_images, const void* rgb_dev, int w, int h, int center, const void* bins_dev,
                           uint64_t n_bits, double alpha, void* bits_out_dev) {
    if (!c || n_images < 0 || !rgb_dev || (n_bits && (!bins_dev || !bits_out_dev))) return TFFT_E_INVALID;
    if (!index_ok(c, n_bits) || !phase_ok(c, n_bits)) return TFFT_E_STATE;
    if (c->ph_adaptive && !(fabs(alpha) < M_PI / 2)) return TFFT_E_INVALID;      // (see extract_chunk)
    const uint8_t* rgb = (const uint8_t*)rgb_dev;
    uint8_t* bits_out = (uint8_t*)bits_out_dev;
    const size_t img_bytes = image_bytes(w, h);
    const ChunkArgs a = ChunkArgs::list(bins_dev, n_bits, alpha);
    std::vector<uint64_t> key = {2, (uint64_t)n_images, key_bits(rgb_dev), (uint64_t)w, (uint64_t)h, (uint64_t)center, key_bits(bins_dev), n_bits,
                                       key_bits(alpha), key_bits(bits_out_dev), key_bits(c->bit_index), key_bits((double)c->dc_bias)};
    phase_key(c, key);
    auto body = [&](const Chunk& k) { return extract_chunk(c, k.s0, k.g, k.st, a, nth(rgb, k.i1, img_bytes), nth(bits_out, k.i1, n_bits)); };
    return with_graph(c, read_is_simple(alpha) ? n_images : 0, key, [&] { return for_chunks(c, n_images, w, h, center, true, nullptr, body); },
                      [&] { return batch_after(c, n_images, w, h, center); });
}

// ---------------------------------------------------------------- packed-byte streams (SURVEY 8 f-3 wired into the pipelines)
// the scratch of the stream calls: the images' payload lengths and, with raw, the raw bits of n_slots whole lists (sized exactly)
static int ensure_stream(tfft_ctx* c, uint64_t n_bins, bool raw = true) {
    if (!c->stream_plen && dev_alloc(c, (void**)&c->stream_plen, (size_t)c->n_slots * sizeof(unsigned))) return TFFT_E_NOMEM;
    const size_t need = raw ? (size_t)c->n_slots * n_bins : 0;
    if (need <= c->stream_cap) return TFFT_OK;
    c->stream_cap = 0;
    int rc = regrow(c, {{(void**)&c->stream_bits, need + 64}});
    if (rc) return rc;
    c->stream_cap = need;
    return TFFT_OK;
}

int tfft_embed_stream_batch_dev(tfft_ctx* c, int n_images, const void* rgb_dev, int w, int h, int center, const void* bins_dev,
                                uint64_t n_bins, const void* header_dev, const void* payload_dev, uint64_t payload_len, double alpha,
                                double rmin, double rmax, double magmin, void* usable_out_dev, void* rgb_out_dev) {
    if (!c || n_images < 0 || !rgb_dev || !rgb_out_dev || !bins_dev || !header_dev || (payload_len && !payload_dev)) return TFFT_E_INVALID;
    if (!stream_fits(n_bins, payload_len)) return TFFT_E_INVALID;
    if (stream_bits(payload_len) > n_bins) return TFFT_E_INVALID;      // the caller's walk is shorter than the stream
    if (!index_ok(c, n_bins) || !phase_ok(c, n_bins)) return TFFT_E_STATE;
    int rc = ensure_stream(c, n_bins);                                // (may reallocate: before any cached sequence is looked up)
    if (rc) return rc;
    // bits_from_bytes + rep3/rep7_encode happen inside k_embed: every bin computes its own stream bit from the packed frame
    const ChunkArgs a = ChunkArgs::list(bins_dev, n_bins, alpha).capacity(rmin, rmax, magmin).frames(header_dev, payload_dev, payload_len);
    EmbedDev e{a, (const uint8_t*)rgb_dev, (uint8_t*)rgb_out_dev, (unsigned long long*)usable_out_dev, bx_begin(c, n_images, usable_out_dev)};
    if (e.bx && c->bx_mode) return embed_chunks(c, n_images, w, h, center, false, e);      // (settling synchronises: never captured or replayed)
    e.bx = nullptr;
    std::vector<uint64_t> key = {3, (uint64_t)n_images, key_bits(rgb_dev), (uint64_t)w, (uint64_t)h, (uint64_t)center, key_bits(bins_dev), n_bins,
                                       key_bits(header_dev), key_bits(payload_dev), payload_len, key_bits(alpha), key_bits(rmin), key_bits(rmax),
                                       key_bits(magmin), key_bits(usable_out_dev), key_bits(rgb_out_dev), key_bits(c->bit_index), key_bits((double)c->dc_bias)};
    phase_key(c, key);
    return with_graph(c, n_images, key, [&] { return embed_chunks(c, n_images, w, h, center, false, e); },
                      [&] { return batch_after(c, n_images, w, h, center); });
}

// The tail of both stream extracts: a chunk's raw bits -> header, payload and status.  Every position of the walk was read in the one pass that
// had the spectrum on chip; the header decides afterwards how many belong to the stream (S:1223-1264: its own bits, clen, then clen+16 bytes' worth)
struct DecodeOut { uint8_t* header; uint8_t* payload; uint64_t max_plen; int* status; };
static int decode_chunk(tfft_ctx* c, const Chunk& k, const uint8_t* raw, uint64_t n_bins, const DecodeOut& o, unsigned* plen) {
    HIPCHK(c, launch_stream_decode(raw, n_bins, o.max_plen, k.g, nth(o.header, k.i1, kHeaderBytes), nth(o.payload, k.i1, o.max_plen), nth(o.status, k.i1),
                                   plen, k.st));
    return TFFT_OK;
}

int tfft_extract_stream_batch_dev(tfft_ctx* c, int n_images, const void* rgb_dev, int w, int h, int center, const void* bins_dev,
                                  uint64_t n_bins, double alpha, void* header_out_dev, void* payload_out_dev, uint64_t max_payload_len,
                                  void* status_out_dev, void* raw_bits_out_dev) {
    if (!c || n_images < 0 || !rgb_dev || !bins_dev || n_bins == 0 || !header_out_dev || !status_out_dev || (max_payload_len && !payload_out_dev))
        return TFFT_E_INVALID;
    if (!index_ok(c, n_bins) || !phase_ok(c, n_bins)) return TFFT_E_STATE;
    if (c->ph_adaptive && !(fabs(alpha) < M_PI / 2)) return TFFT_E_INVALID;      // (see extract_chunk)
    int rc = ensure_stream(c, n_bins, !raw_bits_out_dev);
    if (rc) return rc;
    const uint8_t* rgb = (const uint8_t*)rgb_dev;
    uint8_t* raw_out = (uint8_t*)raw_bits_out_dev;
    const size_t img_bytes = image_bytes(w, h);
    const DecodeOut out{(uint8_t*)header_out_dev, (uint8_t*)payload_out_dev, max_payload_len, (int*)status_out_dev};
    const ChunkArgs a = ChunkArgs::list(bins_dev, n_bins, alpha);
    std::vector<uint64_t> key = {4, (uint64_t)n_images, key_bits(rgb_dev), (uint64_t)w, (uint64_t)h, (uint64_t)center, key_bits(bins_dev), n_bins,
                                       key_bits(alpha), key_bits(header_out_dev), key_bits(payload_out_dev), max_payload_len, key_bits(status_out_dev),
                                       key_bits(raw_bits_out_dev), key_bits(c->bit_index), key_bits((double)c->dc_bias)};
    phase_key(c, key);
    auto body = [&](const Chunk& k) {
        uint8_t* raw = raw_out ? nth(raw_out, k.i1, n_bins) : c->stream_bits;      // (no slot offset: see for_chunks)
        const int rc1 = extract_chunk(c, k.s0, k.g, k.st, a, nth(rgb, k.i1, img_bytes), raw);
        return rc1 ? rc1 : decode_chunk(c, k, raw, n_bins, out, c->stream_plen);
    };
    return with_graph(c, read_is_simple(alpha) ? n_images : 0, key, [&] { return for_chunks(c, n_images, w, h, center, false, nullptr, body); },
                      [&] { return batch_after(c, n_images, w, h, center); });
}

// ---------------------------------------------------------------- host-buffer batches
// The slots are split into a ring of up to four parts; while one part computes, the next parts' inputs
// arrive over PCIe on a copy-in stream and earlier results leave on a copy-out stream.  Overlap needs pinned
// host memory (tfft_host_alloc or any page-locked buffer); pageable buffers work but serialise.
static int pipe_init(tfft_ctx* c) {
    if (c->s_in) return TFFT_OK;
    HIPCHK(c, hipStreamCreateWithFlags(&c->s_in, hipStreamNonBlocking));
    HIPCHK(c, hipStreamCreateWithFlags(&c->s_out, hipStreamNonBlocking));
    for (int i = 0; i < 4; i++) {
        HIPCHK(c, hipEventCreateWithFlags(&c->ev_in[i], hipEventDisableTiming));
        HIPCHK(c, hipEventCreateWithFlags(&c->ev_comp[i], hipEventDisableTiming));
        HIPCHK(c, hipEventCreateWithFlags(&c->ev_out[i], hipEventDisableTiming));
    }
    return dev_alloc(c, (void**)&c->out_pool, (size_t)c->n_slots * c->img_stride_b + 256);
}

// The host arrays of a host-buffer batch call, image i at i times the array's stride; what a call does not use stays nullptr.
// framed: packed-byte framing around the pipeline (tfft_*_stream_batch*) -- header/payload bytes cross PCIe instead of one byte per bit
struct HostIO {
    const uint8_t* rgb = nullptr;
    const uint8_t* bits = nullptr; uint64_t* usable = nullptr; uint8_t* rgb_out = nullptr;      // embed (usable: optional)
    uint8_t* bits_out = nullptr;                                                                 // extract (framed: the raw bits, optional)
    bool framed = false;
    const uint8_t* header_in = nullptr; const uint8_t* payload_in = nullptr;                     // framed embed, ChunkArgs::plen payload bytes per image
    uint8_t* header_out = nullptr; uint8_t* payload_out = nullptr; uint64_t max_plen = 0; int32_t* status_out = nullptr;   // framed extract
};
static int ensure_stream_io(tfft_ctx* c, uint64_t plen) {
    if (c->sio_hdr && plen <= c->sio_plen) return TFFT_OK;
    c->sio_plen = 0;
    const uint64_t cap = grown(plen, 64);
    const size_t n = (size_t)c->n_slots;
    int rc = regrow(c, {{(void**)&c->sio_hdr, n * kHeaderBytes}, {(void**)&c->sio_pay, n * cap}, {(void**)&c->sio_status, n * sizeof(int)}});
    if (rc) return rc;
    c->sio_plen = cap;
    return TFFT_OK;
}

// call: as for the device forms, but bins (and, per_image, jit) are HOST arrays and the bit source's pointers are unused (io has the host
// side; the device side is each ring part's share of the staging buffers).  per_image: lists and jitter travel per part with the images
static int batch_host(tfft_ctx* c, bool embed, int n_images, int w, int h, int center, const ChunkArgs& call, const HostIO& io) {
    const uint64_t n_bits = call.n_bits;
    const bool walks = call.per_image;
    int32_t* bx = embed ? bx_begin(c, n_images, io.usable) : nullptr;
    if (n_images == 0) return TFFT_OK;
    int rc = pipe_init(c);
    if (rc) return rc;
    if (io.framed) {
        rc = ensure_stream_io(c, embed ? call.plen : io.max_plen);
        if (!rc) rc = ensure_stream(c, n_bits, false);
        if (rc) return rc;
    }
    rc = ensure_stage(c, (uint64_t)c->n_slots * n_bits > n_bits ? (uint64_t)c->n_slots * n_bits : n_bits);
    if (rc) return rc;
    rc = batch_geometry(c, c->n_slots, w, h, center);
    if (rc) return rc;
    { const float2* t; rc = get_twiddles(c, c->slots[0].PWi, &t); if (rc) return rc; rc = get_twiddles(c, c->slots[0].PH, &t); if (rc) return rc; }
    const size_t img_bytes = (size_t)w * h * 3;
    // the slots form a ring of up to four parts: copy-in of part k+1..k+3 overlaps the kernels of part k
    const int nhalves = c->n_slots >= 8 ? 4 : (c->n_slots >= 2 ? 2 : 1);
    const int half = c->n_slots / nhalves;
    if (!walks) HIPCHK(c, hipMemcpyAsync(c->stage_bins, call.bins, n_bits * sizeof(tfft_bin), hipMemcpyHostToDevice, c->stream));
    int chunk = 0;
    for (int i0 = 0; i0 < n_images; i0 += half, chunk++) {
        const int g = (n_images - i0 < half) ? n_images - i0 : half;
        const int hh = chunk % nhalves, s0 = hh * half;
        uint8_t* d_bits = (uint8_t*)c->stage_bits + (size_t)s0 * n_bits;
        uint8_t* d_bout = (uint8_t*)c->stage_out + (size_t)s0 * n_bits;
        // copy-in: the half's input buffers are free once the chunk that used them has been computed
        HIPCHK(c, hipStreamWaitEvent(c->s_in, c->ev_comp[hh], 0));
        // the pipeline treats the half's staging area as one packed batch buffer (g images back to back)
        HIPCHK(c, hipMemcpyAsync(c->img(s0), io.rgb + (size_t)i0 * img_bytes, (size_t)g * img_bytes, hipMemcpyHostToDevice, c->s_in));
        tfft_bin* d_bins = (tfft_bin*)c->stage_bins + (walks ? (size_t)s0 * n_bits : 0);
        float* d_jit = (float*)c->stage_jit + (size_t)s0 * n_bits;
        if (walks) {
            HIPCHK(c, hipMemcpyAsync(d_bins, call.bins + (size_t)i0 * n_bits, (size_t)g * n_bits * sizeof(tfft_bin), hipMemcpyHostToDevice, c->s_in));
            if (call.jit) HIPCHK(c, hipMemcpyAsync(d_jit, call.jit + (size_t)i0 * n_bits, (size_t)g * n_bits * sizeof(float), hipMemcpyHostToDevice, c->s_in));
        }
        if (embed && !io.framed) HIPCHK(c, hipMemcpyAsync(d_bits, io.bits + (size_t)i0 * n_bits, (size_t)g * n_bits, hipMemcpyHostToDevice, c->s_in));
        if (embed && io.framed) {      // kHeaderBytes + plen bytes per image instead of stream_bits(plen)
            HIPCHK(c, hipMemcpyAsync(c->sio_hdr + (size_t)s0 * kHeaderBytes, io.header_in + (size_t)i0 * kHeaderBytes, (size_t)g * kHeaderBytes, hipMemcpyHostToDevice, c->s_in));
            if (call.plen) HIPCHK(c, hipMemcpyAsync(c->sio_pay + (size_t)s0 * call.plen, io.payload_in + (size_t)i0 * call.plen, (size_t)g * call.plen, hipMemcpyHostToDevice, c->s_in));
        }
        HIPCHK(c, hipEventRecord(c->ev_in[hh], c->s_in));
        // compute: needs the inputs, and the half's output buffers drained by the copy-out of two chunks ago
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_in[hh], 0));
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_out[hh], 0));
        ChunkArgs a = call;      // the part's device arguments
        a.bins = d_bins; a.jit = walks && call.jit ? d_jit : nullptr;
        if (embed && io.framed) {      // bits_from_bytes + rep3/rep7 inside k_embed, from the packed frames of this part of the ring
            a.hdr = c->sio_hdr + (size_t)s0 * kHeaderBytes; a.pay = c->sio_pay + (size_t)s0 * call.plen;
        } else if (embed) a.bits = d_bits;
        if (embed) {
            rc = embed_chunk(c, s0, g, c->stream, a, c->img(s0), io.usable ? c->usable + s0 : nullptr, c->out_pool + (size_t)s0 * c->img_stride_b);   // packed, like the input
            if (!rc && bx)      // (the part's covers stay in its image buffers until ev_comp)
                rc = bx_settle(c, s0, g, c->img(s0), a, c->usable + s0, bx + i0, c->stream);
        } else
            rc = extract_chunk(c, s0, g, c->stream, a, c->img(s0), d_bout);
        if (rc) return rc;
        if (!embed && io.framed)       // header -> clen -> payload on the device: only packed bytes and a status word go back
            HIPCHK(c, launch_stream_decode(d_bout, n_bits, io.max_plen, g, c->sio_hdr + (size_t)s0 * kHeaderBytes, c->sio_pay + (size_t)s0 * io.max_plen,
                                           c->sio_status + s0, c->stream_plen + s0, c->stream));
        HIPCHK(c, hipEventRecord(c->ev_comp[hh], c->stream));
        // copy-out
        HIPCHK(c, hipStreamWaitEvent(c->s_out, c->ev_comp[hh], 0));
        if (embed) {
            HIPCHK(c, hipMemcpyAsync(io.rgb_out + (size_t)i0 * img_bytes, c->out_pool + (size_t)s0 * c->img_stride_b, (size_t)g * img_bytes, hipMemcpyDeviceToHost, c->s_out));
            if (io.usable) HIPCHK(c, hipMemcpyAsync(io.usable + i0, c->usable + s0, (size_t)g * sizeof(uint64_t), hipMemcpyDeviceToHost, c->s_out));
        } else if (io.framed) {
            HIPCHK(c, hipMemcpyAsync(io.header_out + (size_t)i0 * kHeaderBytes, c->sio_hdr + (size_t)s0 * kHeaderBytes, (size_t)g * kHeaderBytes, hipMemcpyDeviceToHost, c->s_out));
            if (io.max_plen) HIPCHK(c, hipMemcpyAsync(io.payload_out + (size_t)i0 * io.max_plen, c->sio_pay + (size_t)s0 * io.max_plen, (size_t)g * io.max_plen, hipMemcpyDeviceToHost, c->s_out));
            HIPCHK(c, hipMemcpyAsync(io.status_out + i0, c->sio_status + s0, (size_t)g * sizeof(int32_t), hipMemcpyDeviceToHost, c->s_out));
        }
        if (!embed && io.bits_out) HIPCHK(c, hipMemcpyAsync(io.bits_out + (size_t)i0 * n_bits, d_bout, (size_t)g * n_bits, hipMemcpyDeviceToHost, c->s_out));
        HIPCHK(c, hipEventRecord(c->ev_out[hh], c->s_out));
    }
    HIPCHK(c, hipStreamSynchronize(c->s_out));
    return check_err_flag(c);
}

int tfft_embed_batch(tfft_ctx* c, int n_images, const uint8_t* rgb, int w, int h, int center, const tfft_bin* bins,
                     const uint8_t* bits, uint64_t n_bits, double alpha, double rmin, double rmax, double magmin,
                     uint64_t* usable_out, uint8_t* rgb_out) {
    if (!c || n_images < 0 || !rgb || !rgb_out || !bins || !bits || n_bits == 0) return TFFT_E_INVALID;
    const ChunkArgs a = ChunkArgs::list(bins, n_bits, alpha).capacity(rmin, rmax, magmin);
    HostIO io; io.rgb = rgb; io.bits = bits; io.usable = usable_out; io.rgb_out = rgb_out;
    return batch_host(c, true, n_images, w, h, center, a, io);
}
int tfft_extract_batch(tfft_ctx* c, int n_images, const uint8_t* rgb, int w, int h, int center, const tfft_bin* bins,
                       uint64_t n_bits, double alpha, uint8_t* bits_out) {
    if (!c || n_images < 0 || !rgb || !bins || !bits_out || n_bits == 0) return TFFT_E_INVALID;
    const ChunkArgs a = ChunkArgs::list(bins, n_bits, alpha);
    HostIO io; io.rgb = rgb; io.bits_out = bits_out;
    return batch_host(c, false, n_images, w, h, center, a, io);
}
int tfft_embed_stream_batch(tfft_ctx* c, int n_images, const uint8_t* rgb, int w, int h, int center, const tfft_bin* bins, uint64_t n_bins,
                            const uint8_t* header, const uint8_t* payload, uint64_t payload_len, double alpha, double rmin, double rmax,
                            double magmin, uint64_t* usable_out, uint8_t* rgb_out) {
    if (!c || n_images < 0 || !rgb || !rgb_out || !bins || !header || (payload_len && !payload) || n_bins == 0) return TFFT_E_INVALID;
    if (!stream_fits(n_bins, payload_len)) return TFFT_E_INVALID;      // the walk is shorter than the stream
    const ChunkArgs a = ChunkArgs::list(bins, n_bins, alpha).capacity(rmin, rmax, magmin).frames(nullptr, nullptr, payload_len);
    HostIO io; io.rgb = rgb; io.usable = usable_out; io.rgb_out = rgb_out;
    io.framed = true; io.header_in = header; io.payload_in = payload;
    return batch_host(c, true, n_images, w, h, center, a, io);
}
int tfft_extract_stream_batch(tfft_ctx* c, int n_images, const uint8_t* rgb, int w, int h, int center, const tfft_bin* bins, uint64_t n_bins,
                              double alpha, uint8_t* header_out, uint8_t* payload_out, uint64_t max_payload_len, int32_t* status_out,
                              uint8_t* raw_bits_out) {
    if (!c || n_images < 0 || !rgb || !bins || n_bins == 0 || !header_out || !status_out || (max_payload_len && !payload_out)) return TFFT_E_INVALID;
    const ChunkArgs a = ChunkArgs::list(bins, n_bins, alpha);
    HostIO io; io.rgb = rgb; io.bits_out = raw_bits_out;
    io.framed = true; io.header_out = header_out; io.payload_out = payload_out; io.max_plen = max_payload_len; io.status_out = status_out;
    return batch_host(c, false, n_images, w, h, center, a, io);
}
// ---------------------------------------------------------------- one walk per image (own keys, cover-dependent paths)
// The shared-list pipelines above with the lists, jitter and adaptive alpha per image: the buckets are built for the chunk's own lists on
// every call (launch_bucket_walks), the column kernels find image i's buckets at a per-image base (k_fft_cols<..., PI>).  No cached
// sequence (TFFT_GRAPHS) is captured or replayed, and the shared-list state of the context (bit index, phase-option jitter) is refused.
static int walks_args_ok(const tfft_ctx* c, int n_images, uint64_t n_bins, double alpha, int adaptive, bool extract) {
    if (!c || n_images < 0 || n_bins == 0) return TFFT_E_INVALID;
    if (c->bit_index || c->ph_jit) return TFFT_E_STATE;
    if (extract && adaptive && !(fabs(alpha) < M_PI / 2)) return TFFT_E_INVALID;      // (see extract_chunk)
    if ((uint64_t)c->n_slots * n_bins > 0xFFFFFFFFull) return TFFT_E_TOO_LARGE;      // a chunk's entries are addressed with 32 bits
    return TFFT_OK;
}

int tfft_embed_stream_batch_walks_dev(tfft_ctx* c, int n_images, const void* rgb_dev, int w, int h, int center, const void* bins_dev,
                                      const void* jitter_dev, uint64_t n_bins, int adaptive, const void* header_dev, const void* payload_dev,
                                      uint64_t payload_len, double alpha, double rmin, double rmax, double magmin, void* usable_out_dev,
                                      void* rgb_out_dev) {
    if (!c || !rgb_dev || !rgb_out_dev || !bins_dev || !header_dev || (payload_len && !payload_dev)) return TFFT_E_INVALID;
    int rc = walks_args_ok(c, n_images, n_bins, alpha, adaptive, false);
    if (rc) return rc;
    if (!stream_fits(n_bins, payload_len)) return TFFT_E_INVALID;
    const ChunkArgs a = ChunkArgs::list(bins_dev, n_bins, alpha).capacity(rmin, rmax, magmin).frames(header_dev, payload_dev, payload_len)
                            .walks(jitter_dev, adaptive);
    const EmbedDev e{a, (const uint8_t*)rgb_dev, (uint8_t*)rgb_out_dev, (unsigned long long*)usable_out_dev, bx_begin(c, n_images, usable_out_dev)};
    rc = embed_chunks(c, n_images, w, h, center, true, e);
    if (rc) return rc;
    return n_images ? check_err_flag(c) : TFFT_OK;
}

int tfft_extract_stream_batch_walks_dev(tfft_ctx* c, int n_images, const void* rgb_dev, int w, int h, int center, const void* bins_dev,
                                        const void* jitter_dev, uint64_t n_bins, int adaptive, double alpha, void* header_out_dev,
                                        void* payload_out_dev, uint64_t max_payload_len, void* status_out_dev, void* raw_bits_out_dev) {
    if (!c || !rgb_dev || !bins_dev || !header_out_dev || !status_out_dev || (max_payload_len && !payload_out_dev)) return TFFT_E_INVALID;
    int rc = walks_args_ok(c, n_images, n_bins, alpha, adaptive, true);
    if (rc) return rc;
    rc = ensure_stream(c, n_bins, !raw_bits_out_dev);
    if (rc) return rc;
    const uint8_t* rgb = (const uint8_t*)rgb_dev;
    uint8_t* raw_out = (uint8_t*)raw_bits_out_dev;
    const size_t img_bytes = image_bytes(w, h);
    const DecodeOut out{(uint8_t*)header_out_dev, (uint8_t*)payload_out_dev, max_payload_len, (int*)status_out_dev};
    const ChunkArgs a = ChunkArgs::list(bins_dev, n_bins, alpha).walks(jitter_dev, adaptive);
    rc = for_chunks(c, n_images, w, h, center, true, nullptr, [&](const Chunk& k) {
        // (each half of a split chunk has the scratch of its own slots)
        uint8_t* raw = raw_out ? nth(raw_out, k.i1, n_bins) : c->stream_bits + (size_t)k.s0 * n_bins;
        const int rc1 = extract_chunk(c, k.s0, k.g, k.st, a.from(k.i1), nth(rgb, k.i1, img_bytes), raw);
        return rc1 ? rc1 : decode_chunk(c, k, raw, n_bins, out, c->stream_plen + k.s0);
    });
    if (rc) return rc;
    return n_images ? check_err_flag(c) : TFFT_OK;
}

int tfft_embed_stream_batch_walks(tfft_ctx* c, int n_images, const uint8_t* rgb, int w, int h, int center, const tfft_bin* bins, const float* jitter,
                                  uint64_t n_bins, int adaptive, const uint8_t* header, const uint8_t* payload, uint64_t payload_len, double alpha,
                                  double rmin, double rmax, double magmin, uint64_t* usable_out, uint8_t* rgb_out) {
    if (!c || !rgb || !rgb_out || !bins || !header || (payload_len && !payload)) return TFFT_E_INVALID;
    int rc = walks_args_ok(c, n_images, n_bins, alpha, adaptive, false);
    if (rc) return rc;
    if (!stream_fits(n_bins, payload_len)) return TFFT_E_INVALID;
    const ChunkArgs a = ChunkArgs::list(bins, n_bins, alpha).capacity(rmin, rmax, magmin).frames(nullptr, nullptr, payload_len).walks(jitter, adaptive);
    HostIO io; io.rgb = rgb; io.usable = usable_out; io.rgb_out = rgb_out;
    io.framed = true; io.header_in = header; io.payload_in = payload;
    return batch_host(c, true, n_images, w, h, center, a, io);
}
int tfft_extract_stream_batch_walks(tfft_ctx* c, int n_images, const uint8_t* rgb, int w, int h, int center, const tfft_bin* bins, const float* jitter,
                                    uint64_t n_bins, int adaptive, double alpha, uint8_t* header_out, uint8_t* payload_out, uint64_t max_payload_len,
                                    int32_t* status_out, uint8_t* raw_bits_out) {
    if (!c || !rgb || !bins || !header_out || !status_out || (max_payload_len && !payload_out)) return TFFT_E_INVALID;
    int rc = walks_args_ok(c, n_images, n_bins, alpha, adaptive, true);
    if (rc) return rc;
    const ChunkArgs a = ChunkArgs::list(bins, n_bins, alpha).walks(jitter, adaptive);
    HostIO io; io.rgb = rgb; io.bits_out = raw_bits_out;
    io.framed = true; io.header_out = header_out; io.payload_out = payload_out; io.max_plen = max_payload_len; io.status_out = status_out;
    return batch_host(c, false, n_images, w, h, center, a, io);
}

// ---------------------------------------------------------------- fitted embed: stego that survives the crop
// The embed changes bins of the next_pow2 spectrum and the inverse crops back to W x H, which loses much of every change.  For
// 0 < alpha < pi/2 the reader's decision is linear in the pixels (bit 1 <=> Im(F e^{-ij}) >= 0), so "every stream bit reads right" is a set
// of half-spaces, and alternating projections find a point in it: the corrections enforce the side, with a margin, at the listed bins; the
// inverse keeps the W x H support, rounds and clamps.  The unrounded stego is cover + crop(IFFT(D)), D non-zero at the listed bins only,
// so the whole state is one delta per bucket entry (fit_d); only the image the reader sees is rounded.
//   margin floor: mu >= TFFT_FIT_KAPPA * sigma, sigma = sqrt(W*H/24) the standard deviation of Im F of one coefficient under +-1/2 pixel
//   rounding (the reference's unnormalised transform)
#define TFFT_FIT_KAPPA 3.0
static const unsigned kFitMaxBlocks = 64;      // count workgroups per image (partials per image)

static int ensure_fit(tfft_ctx* c, uint64_t n_bins) {
    const uint64_t need = (uint64_t)c->n_slots * n_bins;
    if (!c->fit_part) {
        if (dev_alloc(c, (void**)&c->fit_part, (size_t)c->n_slots * kFitMaxBlocks * 2 * sizeof(unsigned)) ||
            dev_alloc(c, (void**)&c->fit_cnt, (size_t)c->n_slots * 2 * sizeof(unsigned)) ||
            dev_alloc(c, (void**)&c->fit_iters, (size_t)c->n_slots * sizeof(int32_t)) ||
            dev_alloc(c, (void**)&c->fit_wrong, (size_t)c->n_slots * sizeof(uint32_t))) return TFFT_E_NOMEM;
    }
    if (c->fit_d && need <= c->fit_cap) return TFFT_OK;
    c->fit_cap = 0;
    const uint64_t cap = grown(need, 1024);
    int rc = regrow(c, {{(void**)&c->fit_d, cap * sizeof(float2)}, {(void**)&c->fit_mu, cap * sizeof(float)}});
    if (rc) return rc;
    c->fit_cap = cap;
    return TFFT_OK;
}

// the last forward column step of `rgb` writes the values of the chunk's bucketed bins to tb.fl (COLS_EMIT; nothing else is stored
// when the |F|^2 store is available to switch off)
static int fit_forward(tfft_ctx* c, int g, const uint8_t* rgb, hipStream_t st) {
    auto& tb = c->tb[0];
    ColParams em = bucketed_params(c, 0);
    em.em_fl = tb.fl; em.em_pb = tb.pb; em.em_n = 0;
    if (c->stats_m2) { em.em_m2 = 2; em.st_col0 = c->col0_pool; }
    StageMode md; md.fwd_mode = COLS_EMIT; md.fwd = &em; md.walks = true;
    return enqueue_forward(c, 0, g, rgb, st, md);
}

// One chunk of g <= n_slots images in slots [0, g), on the context's stream.  cover: the chunk's covers in buffers nothing writes during
// the call; iters: host, g entries; wrong_dev: device, g entries
static int fit_chunk(tfft_ctx* c, int g, const ChunkArgs& a0, const uint8_t* cover, unsigned long long* usable, int max_iters, double margin,
                     uint8_t* rgb_out, int32_t* iters, uint32_t* wrong_dev) {
    ChunkArgs a = a0;
    a.values();      // F0 of the listed bins is read below: the forward step writes the list (EmbedPath::tile_fuse would not)
    hipStream_t st = c->stream;
    const Slot& s = c->slots[0];
    const tfft_bin* bins = a.bins;
    const float* jit = a.jit;
    const uint64_t n_bins = a.n_bits;
    // iteration 0: the walks embed itself (bucket build, bit and jitter gathers, forward with statistics and capacities, COLS_EMIT of F0)
    int rc = embed_chunk(c, 0, g, st, a, cover, usable, rgb_out);
    if (rc) return rc;
    rc = check_err_flag(c);         // (a bin out of range: the buckets do not describe the lists)
    if (rc) return rc;
    auto& tb = c->tb[0];
    if (!embed_path(c, s, g, a, usable != nullptr).delta) {      // (TFFT_EMBED_DELTA=0) F' was written into the spectrum: no buckets, no F0 in bucket order yet
        const BucketGeom bg = bucket_geom(c, s, g);
        rc = ensure_buckets(c, 0, n_bins, bg.nb, true);
        if (!rc) rc = build_buckets_walks(c, 0, bins, n_bins, g, s, bg, jit, st);
        if (rc) return rc;
        HIPCHK(c, launch_gather_bits_walks(tb.ent, nullptr, a.hdr, a.pay, a.plen, n_bins, a.limit, g, tb.pb, st));
        rc = fit_forward(c, g, cover, st);
        if (rc) return rc;
    }
    const float2* jp = jit ? tb.jp : nullptr;
    const double sigma = sqrt((double)s.W * (double)s.H / 24.0);
    HIPCHK(c, launch_fit_init(tb.ent, tb.fl, tb.pb, jp, bins, a.adaptive ? c->med : nullptr, n_bins, g, a.alpha, margin, TFFT_FIT_KAPPA * sigma,
                              c->fit_d, c->fit_mu, st));
    // a correction of a bin reaches the cropped image with W*H/(PW*PH) of its energy
    const double gain = ((double)s.PW * (double)s.PH) / ((double)s.W * (double)s.H);
    const unsigned nblk = (unsigned)std::min<uint64_t>(kFitMaxBlocks, (n_bins + 1023) / 1024);
    ColParams ed = bucketed_params(c, 0);
    ed.em_fl = c->fit_d; ed.em_pb = tb.pb; ed.em_n = 0;      // (COLS_EMBED_D: em_fl holds the deltas themselves)
    std::vector<unsigned> cnt((size_t)2 * g);
    for (int i = 0; i < g; i++) iters[i] = -1;
    for (int t = 0;; t++) {
        rc = fit_forward(c, g, rgb_out, st);          // F_t of the bytes the reader will see
        if (rc) return rc;
        HIPCHK(c, launch_fit_count(tb.ent, tb.fl, tb.pb, jp, c->fit_mu, n_bins, g, nblk, c->fit_part, c->fit_cnt, wrong_dev, st));
        HIPCHK(c, hipMemcpyAsync(cnt.data(), c->fit_cnt, cnt.size() * sizeof(unsigned), hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        bool all = true;
        for (int i = 0; i < g; i++) {
            if (iters[i] < 0 && cnt[2 * i] == 0 && cnt[2 * i + 1] == 0) iters[i] = t;
            all = all && iters[i] >= 0;
        }
        if (all || t >= max_iters) break;
        // converged images keep their deltas: the inverse gives their bytes again
        HIPCHK(c, launch_fit_correct(tb.ent, tb.fl, tb.pb, jp, c->fit_mu, c->fit_cnt, n_bins, g, gain, c->fit_d, st));
        StageMode mi; mi.inv_mode = COLS_EMBED_D; mi.inv = &ed; mi.walks = true; mi.inv_cover = cover;
        rc = enqueue_inverse(c, 0, g, rgb_out, st, mi);
        if (rc) return rc;
    }
    return TFFT_OK;
}

static int fit_args_ok(const tfft_ctx* c, int n_images, uint64_t n_bins, uint64_t payload_len, double alpha, int adaptive, int max_iters,
                       double margin) {
    int rc = walks_args_ok(c, n_images, n_bins, alpha, adaptive, false);
    if (rc) return rc;
    if (!(alpha > 0.0 && alpha < M_PI / 2) || max_iters < 0 || !(margin > 0.0)) return TFFT_E_INVALID;      // the line-side reading needs 0 < alpha < pi/2
    if (!stream_fits(n_bins, payload_len)) return TFFT_E_INVALID;
    return TFFT_OK;
}

int tfft_embed_stream_batch_fit_dev(tfft_ctx* c, int n_images, const void* rgb_dev, int w, int h, int center, const void* bins_dev,
                                    const void* jitter_dev, uint64_t n_bins, int adaptive, const void* header_dev, const void* payload_dev,
                                    uint64_t payload_len, double alpha, double rmin, double rmax, double magmin, int max_iters, double margin,
                                    void* usable_out_dev, void* iters_out_dev, void* wrong_out_dev, void* rgb_out_dev) {
    if (!c || !rgb_dev || !rgb_out_dev || !bins_dev || !header_dev || (payload_len && !payload_dev)) return TFFT_E_INVALID;
    int rc = fit_args_ok(c, n_images, n_bins, payload_len, alpha, adaptive, max_iters, margin);
    if (rc) return rc;
    rc = ensure_fit(c, n_bins);
    if (rc) return rc;
    const ChunkArgs a = ChunkArgs::list(bins_dev, n_bins, alpha).capacity(rmin, rmax, magmin).frames(header_dev, payload_dev, payload_len)
                            .walks(jitter_dev, adaptive);
    const size_t img_bytes = image_bytes(w, h);
    std::vector<int32_t> iters((size_t)c->n_slots);
    int32_t* bx = bx_begin(c, n_images, usable_out_dev);
    // (The plain chunk loop, not for_chunks: the fit copies every chunk's covers whether or not the capacities are settled, settles against
    // that copy, and uploads the iteration counts after the settling -- the driver would have to learn all three.)
    rc = for_images(n_images, c->n_slots, [&](int i0, int g) -> int {
        rc = batch_geometry(c, g, w, h, center);
        if (rc) return rc;
        // every iteration adds to the ORIGINAL covers: the chunk's own copy in the slots' image buffers (rgb_out may be rgb)
        HIPCHK(c, hipMemcpyAsync(c->img(0), nth((const uint8_t*)rgb_dev, i0, img_bytes), (size_t)g * img_bytes, hipMemcpyDeviceToDevice, c->stream));
        unsigned long long* usable = nth((unsigned long long*)usable_out_dev, i0);
        rc = fit_chunk(c, g, a.from(i0), c->img(0), usable, max_iters, margin, nth((uint8_t*)rgb_out_dev, i0, img_bytes), iters.data(),
                       nth((uint32_t*)wrong_out_dev, i0));
        if (rc) return rc;
        if (bx) { rc = bx_settle(c, 0, g, c->img(0), a, usable, bx + i0, c->stream); if (rc) return rc; }
        if (iters_out_dev) {
            HIPCHK(c, hipMemcpyAsync((int32_t*)iters_out_dev + i0, iters.data(), (size_t)g * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));      // (the host array is reused by the next chunk)
        }
        return TFFT_OK;
    });
    if (rc) return rc;
    return n_images ? check_err_flag(c) : TFFT_OK;
}

// host buffers: a chunk of n_slots images at a time through the staging buffers (covers in out_pool, the stego written over them)
int tfft_embed_stream_batch_fit(tfft_ctx* c, int n_images, const uint8_t* rgb, int w, int h, int center, const tfft_bin* bins, const float* jitter,
                                uint64_t n_bins, int adaptive, const uint8_t* header, const uint8_t* payload, uint64_t payload_len, double alpha,
                                double rmin, double rmax, double magmin, int max_iters, double margin, uint64_t* usable_out, int32_t* iters_out,
                                uint32_t* wrong_out, uint8_t* rgb_out) {
    if (!c || !rgb || !rgb_out || !bins || !header || (payload_len && !payload)) return TFFT_E_INVALID;
    int rc = fit_args_ok(c, n_images, n_bins, payload_len, alpha, adaptive, max_iters, margin);
    if (rc || n_images == 0) return rc;
    rc = pipe_init(c);
    if (!rc) rc = ensure_stage(c, (uint64_t)c->n_slots * n_bins);
    if (!rc) rc = ensure_stream_io(c, payload_len);
    if (!rc) rc = ensure_fit(c, n_bins);
    if (rc) return rc;
    // (every chunk goes through the front of the staging buffers)
    const ChunkArgs a = ChunkArgs::list(c->stage_bins, n_bins, alpha).capacity(rmin, rmax, magmin).frames(c->sio_hdr, c->sio_pay, payload_len)
                            .walks(jitter ? c->stage_jit : nullptr, adaptive);
    const size_t img_bytes = image_bytes(w, h);
    std::vector<int32_t> iters((size_t)c->n_slots);
    int32_t* bx = bx_begin(c, n_images, usable_out);
    hipStream_t st = c->stream;
    const std::vector<HostArray> in = {{rgb, c->img(0), img_bytes}, {bins, c->stage_bins, n_bins * sizeof(tfft_bin)}, {jitter, c->stage_jit, n_bins * sizeof(float)},
                                       {header, c->sio_hdr, kHeaderBytes}, {payload, c->sio_pay, payload_len}};
    const std::vector<HostArray> out = {{rgb_out, c->out_pool, img_bytes}, {usable_out, c->usable, sizeof(uint64_t)}, {wrong_out, c->fit_wrong, sizeof(uint32_t)}};
    rc = for_images(n_images, c->n_slots, [&](int i0, int g) -> int {
        rc = batch_geometry(c, g, w, h, center);
        if (!rc) rc = upload(c, in, i0, g, st);
        if (!rc) rc = fit_chunk(c, g, a, c->img(0), usable_out ? c->usable : nullptr, max_iters, margin, c->out_pool, iters.data(), c->fit_wrong);
        if (!rc && bx) rc = bx_settle(c, 0, g, c->img(0), a, c->usable, bx + i0, st);
        if (!rc) rc = download_sync(c, out, i0, g, st);
        if (!rc && iters_out) memcpy(iters_out + i0, iters.data(), (size_t)g * sizeof(int32_t));
        return rc;
    });
    return rc ? rc : check_err_flag(c);
}

int tfft_lowfreq_mag_batch_dev(tfft_ctx* c, int n_images, const void* rgb_dev, int w, int h, int center, int region, void* out_dev) {
    if (!c || n_images < 0 || !rgb_dev || !out_dev || region < 1 || region > 8) return TFFT_E_INVALID;
    if (n_images == 0) return TFFT_OK;
    Slot s;
    int rc = set_geometry(c, s, w, h, center);
    if (rc) return rc;
    if (region > s.PH || region > s.PW) return TFFT_E_INVALID;
    // the row sums of image k of a chunk in tmp(k), as tfft_lowfreq_mag keeps them (free outside a call: nothing lives there between calls)
    const size_t row_bytes = (size_t)s.H * 3 * region * sizeof(double2), out_len = (size_t)3 * region * region;
    if (row_bytes > c->slot_stride * sizeof(float2)) return TFFT_E_INVALID;
    const size_t img_bytes = image_bytes(w, h);
    return for_images(n_images, c->n_slots, [&](int i0, int g) -> int {
        HIPCHK(c, launch_lowfreq_f64_batch(nth((const uint8_t*)rgb_dev, i0, img_bytes), s.W, s.H, s.PW, s.PH, s.center, region, g, (double2*)c->tmp(0),
                                           c->slot_stride * sizeof(float2) / sizeof(double2), nth((double*)out_dev, i0, out_len), c->stream));
        return TFFT_OK;
    });
}

// ---- stego analysis: annulus phase histograms, cover / stego quality
}  // extern "C"
namespace {
// The analysis scratch, shared by the analysis, robustness and SPAM calls (no call keeps anything in it for the next): grown on demand; an
// earlier call may still read it, so the stream is drained before the old buffer goes.  The replaced buffer leaves tfft_device_bytes.
// (Like bx_value_buffers, no quiesce(): these calls run on the context's stream alone and are never captured.)
int ensure_analysis(tfft_ctx* c, size_t bytes) {
    if (c->an_buf && bytes <= c->an_cap) return TFFT_OK;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    (void)hipFree(c->an_buf); c->an_buf = nullptr; c->dev_bytes -= c->an_cap; c->an_cap = 0;
    const size_t cap = grown(bytes, 4096);
    int rc = dev_alloc(c, &c->an_buf, cap);
    if (rc) return rc;
    c->an_cap = cap;
    return TFFT_OK;
}
// Typed arrays taken off a base pointer one behind the other, each at a multiple of 256 bytes; off a null base the takes only add up
struct Carve {
    char* base; size_t end = 0;
    template <class T> T* take(size_t n) { const size_t at = (end + 255) / 256 * 256; end = at + n * sizeof(T); return base ? (T*)(base + at) : nullptr; }
};
// A call's layout of the scratch, run twice: off a null base for the bytes to ensure, then off the buffer (size and layout cannot drift apart)
template <class Layout> int carve_analysis(tfft_ctx* c, Layout&& layout) {
    Carve size{nullptr};
    layout(size);
    const int rc = ensure_analysis(c, size.end);
    Carve k{(char*)c->an_buf};
    if (!rc) layout(k);
    return rc;
}

int phase_hist_args(tfft_ctx* c, int n_images, const void* rgb, int w, int h, int center, int n_hist_bins, const void* out, int* log_bins) {
    if (!c || n_images < 1 || !rgb || !out || n_hist_bins < 8 || n_hist_bins > 4096 || (n_hist_bins & (n_hist_bins - 1))) return TFFT_E_INVALID;
    Slot s;
    int rc = set_geometry(c, s, w, h, center);
    if (rc) return rc;
    *log_bins = ilog2i(n_hist_bins);
    return TFFT_OK;
}

// g images (device, packed) -> storing forward into slots [0, g) -> histograms, 3*nbins words per image, to hist (device); or, with host
// given, staged in the scratch behind the partials and copied to images [i0, i0+g) of that host array, which synchronises
int phase_hist_chunk(tfft_ctx* c, int g, const uint8_t* rgb, int w, int h, int center, double rmin, double rmax, const double thr[3], int log_bins,
                     uint32_t* hist, uint32_t* host = nullptr, int i0 = 0) {
    int rc = batch_geometry(c, g, w, h, center);
    if (rc) return rc;
    PhaseHistParams P{};
    P.cap = cap_params(c, c->slots[0], rmin, rmax);
    for (int q = 0; q < 3; q++) P.t2[q] = thr ? mag2_threshold(thr[q]) : -INFINITY;
    P.log_bins = log_bins;
    const size_t words = (size_t)3 << log_bins;
    unsigned* part = nullptr;
    rc = carve_analysis(c, [&](Carve& k) {
        part = k.take<unsigned>((size_t)g * phase_hist_blocks(P.cap, log_bins, g) * words);
        if (host) hist = k.take<uint32_t>((size_t)g * words);
    });
    if (rc) return rc;
    rc = enqueue_forward(c, 0, g, rgb, c->stream);      // the storing forward: complex values are needed, not |F|^2
    if (rc) return rc;
    HIPCHK(c, launch_phase_hist(c->spec(0), P, g, part, hist, c->stream));
    return host ? download_sync(c, {{host, hist, words * sizeof(uint32_t)}}, i0, g, c->stream) : TFFT_OK;
}

int quality_args(const tfft_ctx* c, int n_images, const void* a, const void* b, int w, int h, const void* sse, const void* ssim) {
    if (!c || n_images < 1 || !a || !b || !sse || w < 1 || h < 1) return TFFT_E_INVALID;
    if (w > c->max_w || h > c->max_h) return TFFT_E_TOO_LARGE;
    if (ssim && (w < 11 || h < 11)) return TFFT_E_INVALID;
    return TFFT_OK;
}

QualityParams quality_params(int w, int h) {
    QualityParams P{};
    P.W = w; P.H = h;
    double g[11], sum = 0.0;
    for (int k = 0; k < 11; k++) { g[k] = exp(-(double)((k - 5) * (k - 5)) / (2.0 * 1.5 * 1.5)); sum += g[k]; }
    for (int k = 0; k < 11; k++) P.g[k] = (float)(g[k] / sum);
    return P;
}
// the partials of each kind (SSE, SSIM) of the call's largest chunk: one per (image, plane, tile)
size_t quality_tiles(const tfft_ctx* c, int n_images, int w, int h) { return (size_t)(n_images < c->n_slots ? n_images : c->n_slots) * 3 * quality_partials(w, h); }

}  // namespace
extern "C" {

int tfft_phase_hist_batch_dev(tfft_ctx* c, int n_images, const void* rgb_dev, int w, int h, int center, double rmin, double rmax,
                              const double thr[3], int n_hist_bins, void* hist_out_dev) {
    int lb = 0;
    int rc = phase_hist_args(c, n_images, rgb_dev, w, h, center, n_hist_bins, hist_out_dev, &lb);
    if (rc) return rc;
    const size_t img_bytes = image_bytes(w, h), hist_len = (size_t)3 << lb;
    return for_images(n_images, c->n_slots, [&](int i0, int g) {
        return phase_hist_chunk(c, g, nth((const uint8_t*)rgb_dev, i0, img_bytes), w, h, center, rmin, rmax, thr, lb, nth((uint32_t*)hist_out_dev, i0, hist_len));
    });
}

int tfft_phase_hist_batch(tfft_ctx* c, int n_images, const uint8_t* rgb, int w, int h, int center, double rmin, double rmax,
                          const double thr[3], int n_hist_bins, uint32_t* hist_out) {
    int lb = 0;
    int rc = phase_hist_args(c, n_images, rgb, w, h, center, n_hist_bins, hist_out, &lb);
    if (rc) return rc;
    return for_images(n_images, c->n_slots, [&](int i0, int g) {
        drop_images(c, g);      // their images go now (the forward follows)
        rc = upload(c, {{rgb, c->img(0), image_bytes(w, h)}}, i0, g, c->stream);
        return rc ? rc : phase_hist_chunk(c, g, c->img(0), w, h, center, rmin, rmax, thr, lb, nullptr, hist_out, i0);
    });
}

int tfft_quality_batch_dev(tfft_ctx* c, int n_images, const void* a_dev, const void* b_dev, int w, int h, void* sse_out_dev, void* ssim_out_dev) {
    int rc = quality_args(c, n_images, a_dev, b_dev, w, h, sse_out_dev, ssim_out_dev);
    if (rc) return rc;
    const QualityParams P = quality_params(w, h);
    const size_t img_bytes = image_bytes(w, h), nt = quality_tiles(c, n_images, w, h);
    unsigned long long* sse_part = nullptr;
    double* ssim_part = nullptr;
    rc = carve_analysis(c, [&](Carve& k) { sse_part = k.take<unsigned long long>(nt); ssim_part = k.take<double>(nt); });
    if (rc) return rc;
    return for_images(n_images, c->n_slots, [&](int i0, int g) -> int {
        HIPCHK(c, launch_quality(nth((const uint8_t*)a_dev, i0, img_bytes), nth((const uint8_t*)b_dev, i0, img_bytes), P, g, sse_part, ssim_part,
                                 nth((unsigned long long*)sse_out_dev, i0, 3), nth((double*)ssim_out_dev, i0, 3), c->stream));
        return TFFT_OK;
    });
}

// host buffers: a chunk of n_slots pairs at a time, staged OUTSIDE the slots' image buffers (which tfft_lowfreq_mag and the exact statistics
// read again after a single-image forward): the second images in the staging pool of the host pipelines, the first ones in the analysis
// scratch behind the partials and the chunk's results
int tfft_quality_batch(tfft_ctx* c, int n_images, const uint8_t* a, const uint8_t* b, int w, int h, uint64_t* sse_out, double* ssim_out) {
    int rc = quality_args(c, n_images, a, b, w, h, sse_out, ssim_out);
    if (rc) return rc;
    rc = pipe_init(c);
    if (rc) return rc;
    const QualityParams P = quality_params(w, h);
    const size_t img_bytes = image_bytes(w, h), nt = quality_tiles(c, n_images, w, h), g0 = (size_t)(n_images < c->n_slots ? n_images : c->n_slots);
    unsigned long long *sse_part = nullptr, *sse = nullptr;
    double *ssim_part = nullptr, *ssim = nullptr;
    uint8_t* a_stage = nullptr;
    rc = carve_analysis(c, [&](Carve& k) {
        sse_part = k.take<unsigned long long>(nt); ssim_part = k.take<double>(nt);
        sse = k.take<unsigned long long>(g0 * 3); ssim = k.take<double>(g0 * 3); a_stage = k.take<uint8_t>(g0 * img_bytes);
    });
    if (rc) return rc;
    const std::vector<HostArray> in = {{a, a_stage, img_bytes}, {b, c->out_pool, img_bytes}};
    const std::vector<HostArray> out = {{sse_out, sse, 3 * sizeof(uint64_t)}, {ssim_out, ssim, 3 * sizeof(double)}};
    return for_images(n_images, c->n_slots, [&](int i0, int g) -> int {
        rc = upload(c, in, i0, g, c->stream);
        if (rc) return rc;
        HIPCHK(c, launch_quality(a_stage, c->out_pool, P, g, sse_part, ssim_part, sse, ssim_out ? ssim : nullptr, c->stream));
        return download_sync(c, out, i0, g, c->stream);
    });
}

// ---- robustness analysis: channels over a stego batch, and the errors of what the extractor then reads
}  // extern "C"
namespace {
int channel_ok(const tfft_channel& ch) {
    switch (ch.kind) {
        case 0: return TFFT_OK;
        case 1: return (ch.param >= 0.0f && ch.param < INFINITY) ? TFFT_OK : TFFT_E_INVALID;      // (NaN fails the first compare)
        case 2: return (ch.param >= 1.0f && ch.param <= 100.0f && ch.param == floorf(ch.param)) ? TFFT_OK : TFFT_E_INVALID;
        default: return TFFT_E_INVALID;
    }
}
int channel_args(const tfft_ctx* c, int n_images, const void* rgb, int w, int h, const tfft_channel* ch, int n_channels, const void* out) {
    if (!c || n_images < 1 || !rgb || !out || !ch || n_channels < 1 || w < 1 || h < 1) return TFFT_E_INVALID;
    for (int k = 0; k < n_channels; k++) if (channel_ok(ch[k])) return TFFT_E_INVALID;
    if (w > c->max_w || h > c->max_h) return TFFT_E_TOO_LARGE;
    return TFFT_OK;
}
// g packed images (device) through one channel; image 0 of them is image `index0` of the caller's numbering
int channel_chunk(tfft_ctx* c, const tfft_channel& ch, const uint8_t* in, uint8_t* out, int g, int w, int h, uint64_t index0, hipStream_t st) {
    const size_t img_bytes = image_bytes(w, h);
    switch (ch.kind) {
        case 0:
            if (in != out) HIPCHK(c, hipMemcpyAsync(out, in, (size_t)g * img_bytes, hipMemcpyDeviceToDevice, st));
            return TFFT_OK;
        case 1:
            HIPCHK(c, launch_channel_awgn(in, out, (size_t)g * img_bytes, ch.seed, index0 * (uint64_t)img_bytes, ch.param, st));
            return TFFT_OK;
        default:
            HIPCHK(c, launch_channel_jpeg(in, out, w, h, g, (int)ch.param, st));
            return TFFT_OK;
    }
}

// the scratch of the robustness calls: [results of a chunk, n_channels x n_slots x 4 words (host form)] [status] [header] [payload] [attacked images]
struct RobustBufs { uint32_t* res; int* status; uint8_t* hdr; uint8_t* pay; uint8_t* img; };
int robust_bufs(tfft_ctx* c, int n_channels, uint64_t plen, size_t img_bytes, RobustBufs* b) {
    const size_t n = (size_t)c->n_slots;
    return carve_analysis(c, [&](Carve& k) {
        b->res = k.take<uint32_t>((size_t)n_channels * n * 4);
        b->status = k.take<int>(n);
        b->hdr = k.take<uint8_t>(n * kHeaderBytes);
        b->pay = k.take<uint8_t>(n * plen);
        b->img = k.take<uint8_t>(n * img_bytes);
    });
}
int robust_args(const tfft_ctx* c, int n_images, const void* stego, int w, int h, const void* bins, uint64_t n_bins, double alpha, const void* header,
                const void* payload, uint64_t plen, const tfft_channel* ch, int n_channels, const void* result) {
    int rc = channel_args(c, n_images, stego, w, h, ch, n_channels, result);
    if (rc) return rc;
    if (!bins || !header || (plen && !payload) || !stream_fits(n_bins, plen)) return TFFT_E_INVALID;
    if (c->ph_adaptive && !(fabs(alpha) < M_PI / 2)) return TFFT_E_INVALID;      // (see extract_chunk)
    return TFFT_OK;
}
// One chunk through every channel: attack (a copy; `none` reads the stego itself), extract every position of the list, decode for the status,
// count.  stego / hdr / pay: the chunk's own (device); channel k's counts go to res + (k*res_stride)*4, image k.i1 is image index0 of the caller's
int robust_chunk(tfft_ctx* c, const Chunk& k, const ChunkArgs& a, const uint8_t* stego, const uint8_t* hdr, const uint8_t* pay, uint64_t plen,
                 int w, int h, const tfft_channel* ch, int n_channels, uint64_t index0, const RobustBufs& b, uint32_t* res, size_t res_stride) {
    uint8_t* raw = c->stream_bits;      // (no slot offset: the chunks are not split, see for_chunks)
    for (int q = 0; q < n_channels; q++) {
        const uint8_t* att = stego;
        if (ch[q].kind != 0) {
            int rc = channel_chunk(c, ch[q], stego, b.img, k.g, w, h, index0, k.st);
            if (rc) return rc;
            att = b.img;
        }
        int rc = extract_chunk(c, k.s0, k.g, k.st, a, att, raw);
        if (rc) return rc;
        HIPCHK(c, launch_stream_decode(raw, a.n_bits, plen, k.g, b.hdr, b.pay, b.status, c->stream_plen, k.st));
        uint32_t* out = res + (size_t)q * res_stride * 4;
        HIPCHK(c, hipMemsetAsync(out, 0, (size_t)k.g * 4 * sizeof(uint32_t), k.st));
        HIPCHK(c, launch_robust_count(raw, a.n_bits, hdr, pay, plen, b.status, k.g, out, k.st));
    }
    return TFFT_OK;
}
}  // namespace
extern "C" {

int tfft_channel_batch_dev(tfft_ctx* c, int n_images, const void* rgb_dev, int w, int h, const tfft_channel* ch, uint64_t first_image,
                           void* rgb_out_dev) {
    int rc = channel_args(c, n_images, rgb_dev, w, h, ch, 1, rgb_out_dev);
    if (rc) return rc;
    const size_t img_bytes = image_bytes(w, h);
    return for_images(n_images, c->n_slots, [&](int i0, int g) {
        return channel_chunk(c, *ch, nth((const uint8_t*)rgb_dev, i0, img_bytes), nth((uint8_t*)rgb_out_dev, i0, img_bytes), g, w, h,
                             first_image + (uint64_t)i0, c->stream);
    });
}

// host buffers: a chunk of n_slots images at a time, attacked in place in the analysis scratch (the slots' image buffers stay as they are)
int tfft_channel_batch(tfft_ctx* c, int n_images, const uint8_t* rgb, int w, int h, const tfft_channel* ch, uint64_t first_image, uint8_t* rgb_out) {
    int rc = channel_args(c, n_images, rgb, w, h, ch, 1, rgb_out);
    if (rc) return rc;
    const size_t img_bytes = image_bytes(w, h);
    uint8_t* stage = nullptr;
    rc = carve_analysis(c, [&](Carve& k) { stage = k.take<uint8_t>((size_t)(n_images < c->n_slots ? n_images : c->n_slots) * img_bytes); });
    if (rc) return rc;
    return for_images(n_images, c->n_slots, [&](int i0, int g) {
        rc = upload(c, {{rgb, stage, img_bytes}}, i0, g, c->stream);
        if (!rc) rc = channel_chunk(c, *ch, stage, stage, g, w, h, first_image + (uint64_t)i0, c->stream);
        if (!rc) rc = download_sync(c, {{rgb_out, stage, img_bytes}}, i0, g, c->stream);
        return rc;
    });
}

int tfft_robustness_batch_dev(tfft_ctx* c, int n_images, const void* stego_dev, int w, int h, int center, const void* bins_dev, uint64_t n_bins,
                              double alpha, const void* header_dev, const void* payload_dev, uint64_t payload_len, const tfft_channel* channels,
                              int n_channels, uint64_t first_image, void* result_out_dev) {
    int rc = robust_args(c, n_images, stego_dev, w, h, bins_dev, n_bins, alpha, header_dev, payload_dev, payload_len, channels, n_channels, result_out_dev);
    if (rc) return rc;
    if (!index_ok(c, n_bins) || !phase_ok(c, n_bins)) return TFFT_E_STATE;
    const size_t img_bytes = image_bytes(w, h);
    RobustBufs b;
    rc = ensure_stream(c, n_bins);
    if (!rc) rc = robust_bufs(c, 0, payload_len, img_bytes, &b);
    if (rc) return rc;
    const ChunkArgs a = ChunkArgs::list(bins_dev, n_bins, alpha);
    return for_chunks(c, n_images, w, h, center, false, nullptr, [&](const Chunk& k) {
        return robust_chunk(c, k, a, nth((const uint8_t*)stego_dev, k.i1, img_bytes), nth((const uint8_t*)header_dev, k.i1, kHeaderBytes),
                            nth((const uint8_t*)payload_dev, k.i1, payload_len), payload_len, w, h, channels, n_channels, first_image + (uint64_t)k.i1, b,
                            (uint32_t*)result_out_dev + (size_t)k.i1 * 4, (size_t)n_images);
    });
}

// host buffers: a chunk of n_slots stegos at a time in the slots' image buffers, the list, the frames and the chunk's counts in the staging
// buffers of the host pipelines and the analysis scratch
int tfft_robustness_batch(tfft_ctx* c, int n_images, const uint8_t* stego, int w, int h, int center, const tfft_bin* bins, uint64_t n_bins, double alpha,
                          const uint8_t* header, const uint8_t* payload, uint64_t payload_len, const tfft_channel* channels, int n_channels,
                          uint64_t first_image, uint32_t* result_out) {
    int rc = robust_args(c, n_images, stego, w, h, bins, n_bins, alpha, header, payload, payload_len, channels, n_channels, result_out);
    if (rc) return rc;
    if (!index_ok(c, n_bins) || !phase_ok(c, n_bins)) return TFFT_E_STATE;
    const size_t img_bytes = image_bytes(w, h);
    RobustBufs b;
    rc = ensure_stream(c, n_bins);
    if (!rc) rc = ensure_stream_io(c, payload_len);
    if (!rc) rc = ensure_stage(c, n_bins);
    if (!rc) rc = robust_bufs(c, n_channels, payload_len, img_bytes, &b);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(c->stage_bins, bins, n_bins * sizeof(tfft_bin), hipMemcpyHostToDevice, c->stream));
    const ChunkArgs a = ChunkArgs::list(c->stage_bins, n_bins, alpha);
    const std::vector<HostArray> in = {{stego, c->img(0), img_bytes}, {header, c->sio_hdr, kHeaderBytes}, {payload, c->sio_pay, payload_len}};
    std::vector<HostArray> out;      // channel q's counts: n_images x 4 words of the result, n_slots x 4 words of the scratch
    for (int q = 0; q < n_channels; q++) out.push_back({result_out + (size_t)q * n_images * 4, b.res + (size_t)q * c->n_slots * 4, 4 * sizeof(uint32_t)});
    rc = for_chunks(c, n_images, w, h, center, false, nullptr, [&](const Chunk& k) {
        drop_images(c, k.g);      // their images go now
        int rc1 = upload(c, in, k.i1, k.g, k.st);
        if (!rc1) rc1 = robust_chunk(c, k, a, c->img(0), c->sio_hdr, c->sio_pay, payload_len, w, h, channels, n_channels, first_image + (uint64_t)k.i1, b,
                                     b.res, (size_t)c->n_slots);
        if (!rc1) rc1 = download_sync(c, out, k.i1, k.g, k.st);
        return rc1;
    });
    if (rc) return rc;
    return check_err_flag(c);
}

// ---- SPAM steganalysis features: co-occurrence counts of clamped pixel differences, straight from the image bytes
}  // extern "C"
namespace {
int spam_args(const tfft_ctx* c, int n_images, const void* rgb, int w, int h, int t, const void* out) {
    if (!c || n_images < 1 || !rgb || !out || w < 1 || h < 1 || t < 1 || t > 4) return TFFT_E_INVALID;
    if (w > c->max_w || h > c->max_h) return TFFT_E_TOO_LARGE;
    return TFFT_OK;
}
size_t spam_words(int t) { const size_t n = 2 * (size_t)t + 1; return 12 * n * n * n; }
}  // namespace
extern "C" {

// no scratch and no slot: the images are read where they lie (a launch takes at most 65535 of them)
int tfft_spam_batch_dev(tfft_ctx* c, int n_images, const void* rgb_dev, int w, int h, int t, void* counts_out_dev) {
    int rc = spam_args(c, n_images, rgb_dev, w, h, t, counts_out_dev);
    if (rc) return rc;
    const size_t img_bytes = image_bytes(w, h), words = spam_words(t);
    return for_images(n_images, 65535, [&](int i0, int g) -> int {
        HIPCHK(c, launch_spam(nth((const uint8_t*)rgb_dev, i0, img_bytes), w, h, g, t, nth((uint32_t*)counts_out_dev, i0, words), c->stream));
        return TFFT_OK;
    });
}

// host buffers: a chunk of n_slots images at a time, staged in the analysis scratch behind the chunk's counts (the slots' image buffers
// stay as they are)
int tfft_spam_batch(tfft_ctx* c, int n_images, const uint8_t* rgb, int w, int h, int t, uint32_t* counts_out) {
    int rc = spam_args(c, n_images, rgb, w, h, t, counts_out);
    if (rc) return rc;
    const size_t img_bytes = image_bytes(w, h), words = spam_words(t);
    const size_t g0 = (size_t)(n_images < c->n_slots ? n_images : c->n_slots);
    uint32_t* cnt = nullptr;
    uint8_t* stage = nullptr;
    rc = carve_analysis(c, [&](Carve& k) { cnt = k.take<uint32_t>(g0 * words); stage = k.take<uint8_t>(g0 * img_bytes); });
    if (rc) return rc;
    return for_images(n_images, c->n_slots, [&](int i0, int g) -> int {
        rc = upload(c, {{rgb, stage, img_bytes}}, i0, g, c->stream);
        if (rc) return rc;
        HIPCHK(c, launch_spam(stage, w, h, g, t, cnt, c->stream));
        return download_sync(c, {{counts_out, cnt, words * sizeof(uint32_t)}}, i0, g, c->stream);
    });
}

void* tfft_host_alloc(size_t bytes) {
    void* p = nullptr;
    return hipHostMalloc(&p, bytes, 0) == hipSuccess ? p : nullptr;
}
void tfft_host_free(void* p) { if (p) (void)hipHostFree(p); }

int tfft_frame_expand_dev(tfft_ctx* c, int n_images, const void* header_dev, const void* payload_dev, uint64_t payload_len,
                          void* bits_out_dev) {
    if (!c || n_images < 0 || !header_dev || (payload_len && !payload_dev) || !bits_out_dev) return TFFT_E_INVALID;
    if (n_images == 0) return TFFT_OK;
    HIPCHK(c, launch_frame_expand((const uint8_t*)header_dev, (const uint8_t*)payload_dev, payload_len, n_images, (uint8_t*)bits_out_dev,
                                  stream_bits(payload_len), c->stream));
    return TFFT_OK;
}
int tfft_frame_majority_dev(tfft_ctx* c, int n_images, const void* bits_dev, uint64_t payload_len, void* header_out_dev,
                            void* payload_out_dev) {
    if (!c || n_images < 0 || !bits_dev || !header_out_dev || (payload_len && !payload_out_dev)) return TFFT_E_INVALID;
    if (n_images == 0) return TFFT_OK;
    HIPCHK(c, launch_frame_majority((const uint8_t*)bits_dev, payload_len, n_images, (uint8_t*)header_out_dev, (uint8_t*)payload_out_dev, c->stream));
    return TFFT_OK;
}

int tfft_profile_stage(tfft_ctx* c, int n_images, int stage, int reps, const void* rgb_dev, void* rgb_out_dev,
                       const void* bins_dev, const void* bits_dev, void* bits_out_dev, uint64_t n_bits, double alpha,
                       float* ms_per_rep, int* n_launches) {
    if (!c || n_images < 1 || n_images > c->n_slots || reps < 1 || !ms_per_rep || stage < 0 || stage >= N_STAGES) return TFFT_E_INVALID;
    const Slot& s = c->slots[0];
    if (s.PH == 0) return TFFT_E_STATE;
    for (int i = 1; i < n_images; i++) c->slots[i] = s;
    const ColPlan pl = plan_cols(c, s.PH, s.PWi, n_images);
    int launches = 1;
    const int final_fwd = pl.direct ? COLS_FWD_A : COLS_FWD_B;
    if ((stage == COLS_FWD_B || stage == COLS_INV_B) && pl.direct) launches = 0;
    if ((stage == COLS_FWD_A || stage == COLS_INV_B) && pl.fused_fwd) launches = 0;
    if (stage == ROWS_FWD && pl.fused_fwd && c->fuse_live && s.H < s.PH && (s.H % (s.PH >> 3)) != 0) launches = 2;      // one per live-row count
    // The stages are timed the way the pipelines run a chunk of n_images covers with the shared list bins_dev, plain bits and the default
    // capacities: embed_path and read_form say which way that is.  (Delta embedding: no k_embed launch, the first inverse step builds the tiles
    // from the bins and the row kernel adds the cover.  Without bins or bits there is nothing to embed: the stages of the write-F' path)
    const ChunkArgs a = ChunkArgs::list(bins_dev, n_bits, alpha).capacity(0.05, 0.45, 0.01).plain(bits_dev);
    ChunkArgs ae = a;
    if (!bins_dev || !bits_dev) ae.n_bits = 0;
    const EmbedPath path = embed_path(c, s, n_images, ae, true);
    CapParams tcap = cap_params(c, s, a.rmin, a.rmax);
    tcap.magmin = a.magmin;
    // the statistics inside the last forward column step: that step is timed as COLS_STAT; MEDIANS is everything else of the
    // statistics -- sample pass + bracket guess before it, select chain, gated step, fallback and capacity kernels after it
    const bool tile = path.stats == STATS_IN_STEP && (stage == final_fwd || stage == MEDIANS);
    if (stage == COLS_INV_A && path.tile_fuse) launches = 0;      // inside the last forward step's launch
    if (stage == CAPACITY) launches = path.stats == STATS_SEPARATE ? 2 : 0;      // else counted inside the medians' full pass
    if (stage == MEDIANS) {
        // tile: the sample pass and the gated plain step (FFT stages) + the statistics' own kernels around the COLS_STAT step
        if (tile) launches = 2 + stat_tile_launches(stat_opts(c, &tcap, false));
        else launches = plan_medians(s.PH, s.PWi, n_images, stat_opts(c, path.stats == STATS_FUSED ? &tcap : nullptr, path.store == STORE_M2)).launches;
    }
    if (n_launches) *n_launches = launches;
    *ms_per_rep = 0.f;
    if (launches == 0) return TFFT_OK;
    const BucketGeom bg = bucket_geom(c, s, n_images);      // (as embed_chunk and extract_chunk bucket the list)
    { const float2* t; int rc = get_twiddles(c, s.PWi, &t); if (rc) return rc; rc = get_twiddles(c, s.PH, &t); if (rc) return rc; }
    ColParams rd{};
    // COLS_FWD_READ: the last forward step of an extract of a list that is NOT registered, whatever the context has registered (a registered
    // list would move small chunks of large images to the tile-resident read: the stage table keeps the per-call form)
    const bool tile_read = stage == COLS_FWD_READ && read_form(c, s, n_images, a, false) == READ_TILES;
    if (stage == COLS_FWD_READ) {
        if (!bins_dev || !index_ok(c, n_bits)) return TFFT_E_INVALID;
        if (tile_read) {
            if (!bits_out_dev) return TFFT_E_INVALID;
            int rc = ensure_buckets(c, 0, n_bits, bg.nb);
            if (!rc) rc = build_buckets(c, 0, (const tfft_bin*)bins_dev, n_bits, s, bg.G, c->stream);
            if (rc) return rc;
            rd = bucketed_params(c, 0);
            rd.rd_bits = (uint8_t*)bits_out_dev; rd.rd_n = n_bits;
        } else {
            HIPCHK(c, launch_bins_last_row((const tfft_bin*)bins_dev, n_bits, s.PH, s.PWi, c->last_row, c->stream));
            rd.last_row_dev = c->last_row;
        }
    }
    ColParams em{};
    const bool delta_lists = (stage == COLS_INV_A || stage == final_fwd || stage == EMBED || (stage == MEDIANS && tile)) && path.delta;
    if (delta_lists) {
        if (!index_ok(c, n_bits)) return TFFT_E_STATE;
        int rc = ensure_buckets(c, 0, n_bits, bg.nb, true);
        if (rc) return rc;
        rc = build_buckets(c, 0, (const tfft_bin*)bins_dev, n_bits, s, bg.G, c->stream);
        if (rc) return rc;
        const EmbedParams ep0 = embed_params(c, s, n_bits, alpha, 0, nullptr, false);
        em = bucketed_params(c, 0);
        em.em_fl = c->tb[0].fl; em.em_pb = c->tb[0].pb; em.em_n = n_bits;
        em.em_cos = ep0.cos_a; em.em_sin = ep0.sin_a;
        em.em_m2 = path.store;
        if (path.store != STORE_SPEC) em.st_col0 = c->col0_pool;
    }
    // reps back-to-back runs of body() between two events on the context's stream
    auto timed = [&](auto&& body, float* ms) -> int {
        HIPCHK(c, hipEventRecord(c->ev_t0, c->stream));
        for (int r = 0; r < reps; r++) { const int rc = body(); if (rc) return rc; }
        HIPCHK(c, hipEventRecord(c->ev_t1, c->stream));
        HIPCHK(c, hipEventSynchronize(c->ev_t1));
        HIPCHK(c, hipEventElapsedTime(ms, c->ev_t0, c->ev_t1));
        return TFFT_OK;
    };
    if (tile) {
        // phases of enqueue_forward_tilestats: 2 sample + guess, 4 COLS_STAT, 8 select, 16 tail.  The COLS_STAT step alone needs a bracket
        // (one untimed sample pass); MEDIANS = the whole sequence minus the COLS_STAT launches it contains, timed the same way
        float ms_all = 0.f, ms_stat = 0.f;
        // (a fused launch scatters by the stream bits: gathered here, untimed, as the embed stage of the sequence would have before the
        // parent's cols_inv_a -- in bench.py's order that stage comes after this one)
        if (path.tile_fuse) HIPCHK(c, launch_gather_bits(c->tb[0].ent, c->tb[0].off + bg.nb, (const uint8_t*)bits_dev, nullptr, nullptr, 0, n_bits, n_bits, n_images, c->tb[0].pb, c->stream));
        auto run = [&](int phases) { return enqueue_forward_tilestats(c, 0, n_images, (const uint8_t*)rgb_dev, c->stream, em, false, tcap, c->usable, path.tile_fuse, phases); };
        int rc = run(2);
        if (!rc) rc = timed([&] { return run(4); }, &ms_stat);
        if (!rc && stage == MEDIANS) rc = timed([&] { return run(2 | 4 | 8 | 16); }, &ms_all);
        if (rc) return rc;
        *ms_per_rep = (stage == MEDIANS ? (ms_all > ms_stat ? ms_all - ms_stat : 0.f) : ms_stat) / (float)reps;
        return TFFT_OK;
    }
    auto fft_stage = [&](int stg, const StageMode& md) { return enqueue_fft_stage(c, 0, n_images, stg, (const uint8_t*)rgb_dev, (uint8_t*)rgb_out_dev, c->stream, md); };
    float ms = 0.f;
    const int rc = timed([&]() -> int {
        StageMode md;
        switch (stage) {
            case COLS_FWD_A:
            case COLS_FWD_B:
                if (delta_lists && stage == final_fwd) { md.fwd_mode = COLS_EMIT; md.fwd = &em; }
                return fft_stage(stage, md);
            case COLS_INV_A:
                if (delta_lists) { md.inv_mode = COLS_EMBED; md.inv = &em; }
                return fft_stage(stage, md);
            case COLS_INV_B:
            case ROWS_INV:
                if (path.delta && rgb_dev) md.inv_cover = (const uint8_t*)rgb_dev;
                if (path.tile_fuse) { md.inv_mode = COLS_EMBED; md.inv_via_spec = true; }      // the intermediate is where COLS_STAT_EMBED left it
                return fft_stage(stage, md);
            case COLS_FWD_READ:
                md.fwd_mode = tile_read ? COLS_READ : COLS_ROWLIMIT; md.fwd = &rd;
                return fft_stage(final_fwd, md);
            case EMBED:
                if (!index_ok(c, n_bits)) return TFFT_E_STATE;
                // delta embedding: what is left of the embed stage is the gather of the stream bits into bucket order
                if (delta_lists) HIPCHK(c, launch_gather_bits(c->tb[0].ent, c->tb[0].off + bg.nb, (const uint8_t*)bits_dev, nullptr, nullptr, 0, n_bits, n_bits, n_images, c->tb[0].pb, c->stream));
                else HIPCHK(c, launch_embed(c->spec(0), (const tfft_bin*)bins_dev, (const uint8_t*)bits_dev, nullptr, embed_params(c, s, n_bits, alpha, 0, nullptr, false), n_images, c->err, c->stream));
                return TFFT_OK;
            case READ:
                if (!index_ok(c, n_bits)) return TFFT_E_STATE;
                HIPCHK(c, launch_read(c->spec(0), (const tfft_bin*)bins_dev, nullptr, embed_params(c, s, n_bits, alpha, 0, nullptr, false), n_images, (uint8_t*)bits_out_dev, c->err, c->stream));
                return TFFT_OK;
            case MEDIANS:
                if (path.stats == STATS_FUSED) return enqueue_medians(c, 0, n_images, c->stream, &tcap, c->usable, path.store == STORE_M2);
                return enqueue_medians(c, 0, n_images, c->stream);
            case CAPACITY:
                HIPCHK(c, launch_capacity(c->spec(0), tcap, n_images, c->med, c->partial, c->usable, c->stream, nullptr));
                return TFFT_OK;
            default: return fft_stage(stage, md);
        }
    }, &ms);
    *ms_per_rep = ms / (float)reps;
    return rc;
}

// ---------------------------------------------------------------- (f-4) fp64 audit transform
static int audit_run(tfft_ctx* c, double* host, const uint8_t* rgb, int w, int h, int center, int n_planes, int ph, int pw, int inverse) {
    const size_t bytes = (size_t)n_planes * ph * pw * sizeof(double2);
    double2 *a = nullptr, *scratch = nullptr, *wtab = nullptr;
    uint8_t* img = nullptr;
    int rc = TFFT_OK;
    auto done = [&](int r) { (void)hipFree(a); (void)hipFree(scratch); (void)hipFree(wtab); (void)hipFree(img); return r; };
    if (hipMalloc((void**)&a, bytes) != hipSuccess || hipMalloc((void**)&scratch, bytes) != hipSuccess ||
        hipMalloc((void**)&wtab, (size_t)(ph > pw ? ph : pw) * sizeof(double2)) != hipSuccess) return done(TFFT_E_NOMEM);
    hipError_t e;
    if (rgb) {
        const size_t ib = (size_t)w * h * 3;
        if (hipMalloc((void**)&img, ib) != hipSuccess) return done(TFFT_E_NOMEM);
        e = hipMemcpyAsync(img, rgb, ib, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = audit_load_rgb8_f64(img, w, h, pw, ph, center, a, c->stream);
    } else {
        e = hipMemcpyAsync(a, host, bytes, hipMemcpyHostToDevice, c->stream);
    }
    if (e == hipSuccess) e = audit_fft2d_f64(a, scratch, wtab, n_planes, ph, pw, inverse, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(host, a, bytes, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { c->last_hip = (int)e; rc = TFFT_E_HIP; }
    return done(rc);
}
static bool is_pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }

int tfft_audit_fft2d_f64(tfft_ctx* c, double* planes, int n_planes, int ph, int pw, int inverse) {
    if (!c || !planes || n_planes < 1 || !is_pow2(ph) || !is_pow2(pw) || ph > TFFT_MAX_DIM || pw > TFFT_MAX_DIM) return TFFT_E_INVALID;
    return audit_run(c, planes, nullptr, 0, 0, 0, n_planes, ph, pw, inverse);
}

int tfft_audit_forward_rgb8_f64(tfft_ctx* c, const uint8_t* rgb, int w, int h, int center, double* out) {
    if (!c || !rgb || !out || w < 1 || h < 1 || w > TFFT_MAX_DIM || h > TFFT_MAX_DIM) return TFFT_E_INVALID;
    int pw = 1, ph = 1;
    while (pw < w) pw <<= 1;
    while (ph < h) ph <<= 1;
    return audit_run(c, out, rgb, w, h, center, 3, ph, pw, 0);
}

int tfft_timer_begin(tfft_ctx* c) {
    if (!c) return TFFT_E_INVALID;
    HIPCHK(c, hipEventRecord(c->ev_t0, c->stream));
    return TFFT_OK;
}
int tfft_timer_end(tfft_ctx* c, float* ms) {
    if (!c || !ms) return TFFT_E_INVALID;
    HIPCHK(c, hipEventRecord(c->ev_t1, c->stream));
    HIPCHK(c, hipEventSynchronize(c->ev_t1));
    HIPCHK(c, hipEventElapsedTime(ms, c->ev_t0, c->ev_t1));
    return TFFT_OK;
}

}  // extern "C"
