// tfft_kernels.h -- parameter blocks and launchers of tfft_kernels.hip, tfft_stats.hip, tfft_exact.hip and tfft_audit64.hip: the one
// header tfft_capi.hip sees
#pragma once
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "../../include/turtlefft_hip.h"

namespace tfft {

struct RowParams {
    int W, H;        // image size (pixels)
    int PW, PH;      // padded size (internal PW >= 2)
    int center;      // (-1)^(x+y) pre/post multiply (apply_center)
    float scale;     // inverse only: 1/((PW/2)*PH)
    size_t img_stride;   // float2 elements between consecutive images of a batch in tmp/spec
    float bias;          // forward only: subtracted from every pixel before the transform (its rank-1 transform is added
                         // back by the last column step, ColParams::dc_*); 0 = off
    const uint8_t* cover;    // inverse only, delta embedding: the transform holds IFFT(F' - F) and the pixel is
                             // clamp(round(cover + delta)) (images W*H*3 bytes apart, like the output); nullptr = off, bias is added
};

// a bin of the list, located inside its column tile: value at LDS row `k` (= y / G), column `c` (= x % 16)
struct TileBin { uint16_t k; uint8_t c; uint8_t conj; uint32_t bit; };

// The modes of a column step (k_fft_cols; what each does: the comment above the kernel).  The caller of launch_cols names the mode; the
// groups of ColParams below say which mode reads them
enum { COLS_PLAIN = 0, COLS_ROWLIMIT = 1, COLS_READ = 2, COLS_EMBED = 3, COLS_EMIT = 4, COLS_STAT = 5, COLS_EMBED_D = 6, COLS_STAT_EMBED = 7 };
constexpr bool embed_mode(int mode) { return mode == COLS_EMBED || mode == COLS_EMBED_D; }      // the first inverse step of a delta embed
#define TFFT_TILE_FUSE_MIN_LOG 5      // COLS_STAT_EMBED exists from L = 32 on (at L = 16 it holds fewer workgroups per CU than COLS_STAT)
constexpr bool stat_mode(int mode) { return mode == COLS_STAT || mode == COLS_STAT_EMBED; }      // the statistics' bracket pass inside the last forward step

// one column step as launch_cols runs it
struct ColStep {
    int logl;          // log2 of the column length of the step, <= 9
    int sign;          // +1 forward, -1 inverse
    int mode;          // COLS_*
    bool walks;        // the bucket modes with one walk per image (launch_bucket_walks layout, k_fft_cols<..., PI = true>); false: one shared list
};

struct ColParams {
    // every mode: the geometry of the step
    int M;             // columns of the half spectrum (PW/2)
    int PH;            // full column length (twiddle table size)
    int G;             // groups (1 for the direct pass, N2 or N1 for the two-step passes)
    int in_a, in_b;    // input row  = in_a*l  + in_b*g
    int out_a, out_b;  // output row = out_a*k + out_b*g
    int in_rows;       // input rows >= in_rows are zero (not loaded)
    int out_rows;      // output rows >= out_rows are not stored
    // the bucket modes (COLS_READ, COLS_EMIT, COLS_STAT, COLS_EMBED, COLS_EMBED_D): rd_bins, rd_off and trash
    // COLS_READ, extraction straight out of the tiles (the spectrum is never stored): rd_bits, rd_n
    const struct TileBin* rd_bins;   // bins bucketed by (plane, 16-column tile, group g), see k_bucket_*
    const unsigned* rd_off;          // bucket b = (plane*G + g)*ntiles + tile holds rd_bins[rd_off[b] .. rd_off[b+1])
    uint8_t* rd_bits;                // bits_out, image i at rd_bits + i*rd_n
    uint64_t rd_n;
    uint8_t* trash;                  // >= 8 KiB of device scratch nobody reads: where lanes WITHOUT a list entry send their (unpredicated) stores
    // delta embedding: the LAST forward step (COLS_EMIT, COLS_STAT) writes the values of the bucketed bins (rd_bins / rd_off as above) to
    // em_fl in bucket order; the FIRST inverse step (COLS_EMBED) starts every tile as zeros and puts F' - F at those bins, F taken from
    // em_fl (S:712-732 with a fixed alpha); COLS_EMBED_D takes F' - F itself from em_fl, in stored coordinates (the fitted embed)
    float2* em_fl;                   // em_n values per image, indexed like rd_bins
    int em_m2;                       // COLS_EMIT: store |F|^2 (float, `out` reinterpreted, same byte offset per image) instead of the complex
                                     // spectrum, the packed column 0 to st_col0: all the statistics read (launch_medians, StatOpts::m2)
    const uint8_t* em_pb;            // COLS_EMBED: em_n stream bits per image in the same order (k_gather_bits; 2 = not written)
    uint64_t em_n;                   // list stride between images (the length of the bin list; 0 with ColStep::walks, whose entry indices are absolute)
    float em_cos, em_sin;            // COLS_EMBED
    // phase options of the batched calls (tfft_set_phase_options); COLS_EMBED and COLS_READ only
    const float2* em_jp;             // jitter as unit phasors (cos j, sin j), indexed like rd_bins (shared by all images); nullptr = no jitter
    const float* em_med;             // COLS_EMBED, adaptive alpha: 3 medians |F| per image of the launch; nullptr = the fixed em_cos / em_sin
    float em_alpha;                  // ... and the alpha they scale (S:704-710)
    // COLS_STAT_EMBED: COLS_STAT and COLS_EMBED in one visit per tile -- reads `in`, writes the first inverse step's output to `out`; the st_*
    // fields of COLS_STAT, em_pb / em_cos / em_sin / em_jp of COLS_EMBED; em_fl only for bucket entries beyond those a thread keeps in registers
    // statistics inside the last forward step (COLS_STAT = COLS_EMIT without the spectrum store): every value is classified against
    // the bracket of its plane's SelectState exactly as k_collect_bracket does (weight below, candidates, capacity counts, parked
    // values); the packed column 0 goes to st_col0 for k_col0_stats
    struct SelectState* st_sel;      // 3 per image
    unsigned* st_cand; size_t st_cand_stride;
    unsigned st_resv;           // COLS_STAT: slots of the candidate list each wave of the launch owns (set by the launcher: 64 per tile it walks)
    unsigned st_cand_fixed;     // COLS_STAT: slots at the head of a plane's list owned by the launch's waves (set by the launcher); appended entries follow
    unsigned* st_partial;            // per (image, plane) TFFT_STAT_MAX_BLOCKS counters (a workgroup adds to slot block % that)
    float* st_amb;
    float2* st_col0;                 // per (image, plane) PH values
    unsigned st_slo, st_shi;         // squared radius bounds of the annulus, clamped to 32 bits
    int st_cap, st_PW;               // (st_PW: written, not read)
    // forward COLS_PLAIN only: a sample of the tiles (0, tile_step, 2*tile_step, ..) written side by side into a narrow spectrum
    int tile_step, tile_off; int out_M; size_t out_plane_stride, out_img_stride;      // tiles tile_off + i*tile_step
    // forward COLS_PLAIN only: images whose statistics were settled without the spectrum (all three planes) return at once
    const struct SelectState* gate;
    // forward COLS_PLAIN sample pass: instead of storing the narrow spectrum, every value's |F|^2 goes into a 4096-bucket histogram (the
    // top 13 bits of the float, weight 2) kept in LDS at byte offset hist_lds_off and added to hist_sel[3*img + plane].hist at the end
    struct SelectState* hist_sel; unsigned hist_lds_off;
    int g_step, g_off;          // ... and only the row groups g_off + i*g_step of the launch (0: all): rows g + G*k, a regular subsample of the rows
    // DC removal (every forward mode, final step only; inverse: COLS_PLAIN, first step): out[row][col] += dc_ah[row] * dc_aw[col] -- the
    // transform of the constant that the row kernels subtracted from the pixels, c*A_H(y)*A_W(x); nullptr = off
    const float2* dc_ah;       // PH entries, the factor c included
    const float2* dc_aw;       // M entries, entry 0 packed: A_W(0) + i*A_W(M)
    const int* last_row_dev;   // COLS_ROWLIMIT: device scalar, rows > *last_row_dev are not stored either (extraction reads
                               // only the rows its bin list touches; k_bins_last_row)
    // every mode
    int tw_out;        // multiply output by exp(sign*2*pi*i*k*g/PH)
    int tiles_per_block;  // adjacent 16-column tiles walked by one workgroup
    size_t plane_stride;  // float2 elements between planes (PH*M)
    size_t img_stride;    // float2 elements between images (grid.z = 3*n_images)
};

struct EmbedParams {
    uint64_t n;
    int PH, PW;
    int generic;       // 0: alpha fixed, no jitter, 0<alpha<pi -> cos/sin constants and sign test
    int adaptive;
    float cos_a, sin_a;
    double alpha;
    double med[3];
    size_t img_stride;     // float2 elements between images (grid.y = image)
    const uint32_t* bit_index;   // bins[i] carries stream bit bit_index[i] (nullptr: bit i); tfft_set_bit_index
    uint64_t limit;              // embed only: stream bits >= limit are not written (the stream is shorter than the bin list)
    // embed only, stream pipelines: the bits come straight out of the packed frame (38-byte header, frame_plen payload bytes per image)
    const uint8_t* frame_hdr; const uint8_t* frame_pay; uint64_t frame_plen;
    const float* med_dev;        // adaptive, batched calls: 3 medians per image on the device (image i at med_dev + 3*i) instead of med[]
    uint64_t bins_stride;        // one walk per image: image i's bins (and jitter) at bins + i*bins_stride; 0 = one list shared by every image
};

struct CapParams {
    int PH, PW;                     // padded grid as the reference sees it
    int PWi;                        // internal (even) row length used for indexing the half spectrum
    int bw, bh;                     // bounding box of the annulus (x < bw, y < bh)
    unsigned long long s_lo, s_hi;  // s_lo <= y*y+x*x <= s_hi  <=>  rmin*mn <= hypot(y,x) <= rmax*mn
    double magmin;                  // used with med_dev (batch path)
    double thr[3];                  // used when med_dev == nullptr (tfft_capacity)
    size_t img_stride;
};

// Smallest float m2 with (double)sqrtf(m2) >= thr, i.e. the reference's test !(|F| < thr) (S:1004) moved
// onto the argument of mag_of's square root: sqrtf is correctly rounded and monotone, so
// !((double)sqrtf(m2) < thr)  <=>  !(m2 < T2).  One scalar search per thread (wave uniform) replaces a
// correctly rounded square root and a double compare per bin.
__host__ __device__ inline float mag2_threshold(double thr) {
    if (!(thr > 0.0)) return -INFINITY;                 // thr <= 0 or NaN: nothing is ever "< thr"
    float tf = (float)thr;                              // tf = smallest float >= thr
    if ((double)tf < thr) tf = nextafterf(tf, INFINITY);
    if (!(tf < INFINITY)) return INFINITY;
    float c = tf * tf;
    if (!(c < INFINITY)) c = FLT_MAX;
    for (int i = 0; i < 8 && !(sqrtf(c) < tf); i++) c = nextafterf(c, -INFINITY);   // now sqrtf(c) < tf (or c ran to 0)
    for (int i = 0; i < 16 && sqrtf(c) < tf; i++) c = nextafterf(c, INFINITY);      // first value that passes
    return c;
}

// ---- exact medians / capacity of the single-image calls (tfft_exact.hip)
struct ExactCand { uint16_t y, x, w, plane; float m2; };      // a full-grid bin (x = PW/2: the Nyquist column out of the packed column 0), the
                                                              // weight it carries (itself and / or its Hermitian mirror) and its fp32 |F|^2
struct ExactCollect {
    int PH, PW;                       // padded grid (PW = the internal even row length)
    int PW_full;                      // the reference's PW (mirror columns are PW_full - x)
    int cap;                          // 0: median mode, 1: capacity mode (annulus s_lo <= y*y + x*x <= s_hi, axes excluded)
    unsigned long long s_lo, s_hi;
    float lo2[3], hi2[3];             // per plane: window of fp32 |F|^2 whose bins are re-evaluated in fp64
    int cap_cand;                     // candidate slots per plane
};
hipError_t launch_exact_collect(const float2* spec, const ExactCollect& P, ExactCand* cand, unsigned long long* below, unsigned* n_cand, hipStream_t s);
hipError_t launch_exact_table(double2* table, int PW, hipStream_t s);
hipError_t launch_exact_eval(const uint8_t* rgb, int W, int H, int PW, int PH, int center, const ExactCand* cand, unsigned n, int n_split,
                             const double2* table, double2* out, hipStream_t s);
// ... and their batched form (tfft_set_batch_exact): many images of one geometry per launch, each with its own windows
struct ExactCandB { uint16_t y, x, w, plane; float m2; uint32_t img; };      // ExactCand + the image (index into the launch's covers / spectra)
struct ExactWin { int img; float lo2[3], hi2[3]; int rsv; };                 // collect launch entry z: which image, its per-plane |F|^2 windows
struct ExactVal { double re, im; float m2; uint32_t w; };                    // a settled candidate: fp64 F (partials added in order), fp32 |F|^2, weight
struct ExactGroup { unsigned first, count; };                                  // k_exact_eval_batch workgroup: dense candidates [first, first + count)
#define TFFT_EXACT_K 8                // candidates of one (image, plane) per k_exact_eval_batch workgroup: one pixel load serves all of them
// grid (rows, 3, n_win): candidates of entry z, plane p at cand + (3z+p)*P.cap_cand, counters at below / n_cand [3z+p]
hipError_t launch_exact_collect_batch(const float2* spec, size_t img_stride, const ExactCollect& P, const ExactWin* win, int n_win, ExactCandB* cand,
                                      unsigned long long* below, unsigned* n_cand, hipStream_t s);
// groups: n_groups x (first dense index, count 1..TFFT_EXACT_K) into idx[] (-> cand[]), all of one (image, plane); out = n_dense * n_split partials
hipError_t launch_exact_eval_batch(const uint8_t* rgb, size_t img_bytes, int W, int H, int PW, int PH, int center, const ExactCandB* cand,
                                   const unsigned* idx, const ExactGroup* groups, unsigned n_groups, int n_split, const double2* table, double2* out, hipStream_t s);
// out[i] = the n_split partials of dense candidate i added in order (as the single-image host loop adds them) + its m2 and weight
hipError_t launch_exact_sum_batch(const double2* part, int n_split, const ExactCandB* cand, const unsigned* idx, unsigned n, ExactVal* out, hipStream_t s);

#define TFFT_STAT_MAX_BLOCKS 512

struct SelectState {        // one per (image, plane)
    unsigned hist[4096];
    unsigned long long rank;
    unsigned long long below;   // fast path: exact weight of everything below the bracket
    unsigned prefix;
    unsigned n_cand;
    unsigned lo, hi;            // fast path: bracket of level-1 buckets around the sample median
    unsigned done;              // 0 open / fallback needed, 2 fast path verified at level 2, 1 median written
    unsigned fast;              // 1: the median came from the fast path (set with done = 1 by k_select_fast<3>)
    // capacity counted inside the bracket pass (batch path): the threshold T2 = mag2_threshold(magmin * median) is only
    // known afterwards, but the bracket pins it to [t2_lo, t2_hi]: bins at or above t2_hi count now, bins below t2_lo
    // never, the few in between are parked (their |F|^2, once per full-grid bin) and settled by k_capacity_settle
    float t2_lo, t2_hi;
    unsigned n_amb;             // parked values (may exceed TFFT_AMB_CAP: then the plane falls back to k_capacity)
    unsigned cand_fixed;        // slots at the head of the candidate list owned by COLS_STAT's waves (holes included); appended entries follow
};
#define TFFT_AMB_CAP 8192
#define TFFT_CAND_HOLE 0x7FFFFFFFu      // an unused slot of the candidate list (COLS_STAT reserves slots per wave): weight bit clear, a value no bracket reaches

hipError_t launch_rows_fwd(const uint8_t* rgb, float2* out, const float2* tw_pw, const RowParams& P, int n_images,
                           hipStream_t s);
hipError_t launch_rowcol_fwd(const uint8_t* rgb, float2* out, const float2* tw_pw, const float2* tw_ph, const RowParams& P,
                             int n_images, hipStream_t s);
hipError_t launch_colrow_inv(const float2* in, uint8_t* rgb, const float2* tw_pw, const RowParams& P, int n_images, hipStream_t s);
// the forward stage with threads and LDS for the LIVE rows of every group only (one launch per distinct live-row count)
hipError_t launch_rowcol_fwd_live(const uint8_t* rgb, float2* out, const float2* tw_pw, const float2* tw_ph, const RowParams& P, int n_images, hipStream_t s);
hipError_t launch_rows_inv(const float2* in, uint8_t* rgb, const float2* tw_pw, const RowParams& P, int n_images,
                           hipStream_t s);
hipError_t launch_cols(const float2* in, float2* out, const float2* tw_ph, const ColParams& P, const ColStep& step, int n_planes, hipStream_t s);
// (f-4) fp64 audit transform, tfft_audit64.hip
hipError_t audit_fft2d_f64(double2* a, double2* scratch, double2* wtab, int n_planes, int PH, int PW, int inverse, hipStream_t s);
hipError_t audit_load_rgb8_f64(const uint8_t* rgb_dev, int W, int H, int PW, int PH, int center, double2* out, hipStream_t s);
// bucket the bin list by (plane, 16-column tile, row group y % G) for the tile-resident read: counts -> offsets -> entries
hipError_t launch_bucket_bins(const tfft_bin* bins, const uint32_t* bit_index, uint64_t n, int PH, int PW, int G,
                              unsigned* cnt, unsigned* off, TileBin* out, int* err, int force_global, hipStream_t s);
// one walk per image: n_images lists of n bins (image i's at bins + i*n, no bit index) bucketed by (image, plane, group, column tile).
// Image i owns buckets [i*nb, (i+1)*nb), nb = 3*ntiles*G, and bucket n_images*nb holds the invalid bins of all (the error flag is
// raised for those), so that image i's entries are exactly [i*n, (i+1)*n) for valid lists; TileBin::bit = the position in the image's own
// list.  cnt / off hold n_images*nb + 2 words (+ the scan's block totals)
hipError_t launch_bucket_walks(const tfft_bin* bins, uint64_t n, int n_images, int PH, int PW, int G, unsigned* cnt, unsigned* off, TileBin* out,
                               int* err, hipStream_t s);
// ... and the stream bits / the jitter phasors of those entries (entry e belongs to image e / n; bits and jitter at image*n + bit)
hipError_t launch_gather_bits_walks(const TileBin* ent, const uint8_t* bits, const uint8_t* hdr, const uint8_t* pay, uint64_t plen, uint64_t n,
                                    uint64_t limit, int n_images, uint8_t* out, hipStream_t s);
hipError_t launch_gather_jitter_walks(const TileBin* ent, const float* jitter, uint64_t n, int n_images, float2* out, hipStream_t s);
// the fitted embed, over the n_images*n entries of a chunk's walks (fl: the values a COLS_EMIT step wrote, pb: the
// bits, jp: jitter phasors or nullptr, med: 3 medians per image for adaptive alpha or nullptr):
//   init   : d = F' - F0 (stored coordinates), mu = max(tau |F0| sin(alpha_k), mu_floor)
//   count  : per image, entries that read wrong and entries below mu/2 -> counts[2*img], counts[2*img + 1] (and wrong_out[img] if given);
//            nblk workgroups per image, partial = n_images*nblk*2 words
//   correct: images whose counts are not both 0: d += gain * i e^{ij} (s*mu - u) where s*u < mu
hipError_t launch_fit_init(const TileBin* ent, const float2* fl, const uint8_t* pb, const float2* jp, const tfft_bin* bins, const float* med,
                           uint64_t n, int n_images, double alpha, double tau, double mu_floor, float2* d, float* mu, hipStream_t s);
hipError_t launch_fit_count(const TileBin* ent, const float2* fl, const uint8_t* pb, const float2* jp, const float* mu, uint64_t n, int n_images,
                            unsigned nblk, unsigned* partial, unsigned* counts, uint32_t* wrong_out, hipStream_t s);
hipError_t launch_fit_correct(const TileBin* ent, const float2* fl, const uint8_t* pb, const float2* jp, const float* mu, const unsigned* counts,
                              uint64_t n, int n_images, double gain, float2* d, hipStream_t s);
// highest stored row any bin of the list touches -> *last_row (device int, reset here)
hipError_t launch_gather_bits(const TileBin* ent, const unsigned* n_ent, const uint8_t* bits, const uint8_t* hdr, const uint8_t* pay, uint64_t plen,
                              uint64_t n, uint64_t limit, int n_images, uint8_t* out, hipStream_t s);
// jitter (stream order) gathered into bucket order as unit phasors: out[e] = (cos, sin)(jitter[ent[e].bit]), e < *n_ent
hipError_t launch_gather_jitter(const TileBin* ent, const unsigned* n_ent, const float* jitter, uint64_t n, float2* out, hipStream_t s);
hipError_t launch_bins_last_row(const tfft_bin* bins, uint64_t n, int PH, int PW, int* last_row, hipStream_t s);
hipError_t launch_embed(float2* spec, const tfft_bin* bins, const uint8_t* bits, const float* jitter,
                        const EmbedParams& P, int n_images, int* err, hipStream_t s);
hipError_t launch_read(const float2* spec, const tfft_bin* bins, const float* jitter, const EmbedParams& P,
                       int n_images, uint8_t* bits_out, int* err, hipStream_t s);
// ---- the statistics stage (tfft_stats.hip): medians of |F| per plane and, counted in the same pass, the capacities
// the device buffers of the images of one launch (tfft_capi.hip: stat_bufs)
struct StatBufs {
    SelectState* st;                // 3 per image
    unsigned* cand; size_t cand_stride;      // candidate lists, one per plane
    float* med;                     // out: 3 medians per image
    unsigned* partial;              // [n_images*3*TFFT_STAT_MAX_BLOCKS] block counts of the capacity + one flag per image
    float* amb;                     // [n_images*3*TFFT_AMB_CAP] parked |F|^2
    unsigned long long* usable;     // out: the capacities (with StatOpts::cap)
    float2* col0;                   // [n_images*3*PH] packed columns 0 beside |F|^2 planes (StatOpts::m2) and of the COLS_STAT step
};
struct StatOpts {
    const CapParams* cap;           // nullptr: medians only
    bool m2;                        // the spectrum holds |F|^2 planes (ColParams::em_m2), the packed columns 0 are in StatBufs::col0
    int compact;                    // 0: never the compact pipeline (TFFT_STATS_COMPACT)
    int force_fallback;             // skip the fast path (TFFT_MEDIAN_FALLBACK)
    int skew;                       // test hook (TFFT_STATS_SKEW): move the brackets so that the fast path fails
    int fill_cus, fill_resident;    // CUs and resident k_collect_bracket blocks per CU (collect_bracket_resident_blocks); <= 0: 256, 4
};
// planes up to this many bins take the compact pipeline, and only those can be read as |F|^2 planes or settled inside the column step
#define TFFT_COMPACT_MAX_BINS (1ull << 24)
// ... and up to this many bins, in launches of so many images at most, its merged finish kernel
#define TFFT_FINISH1_MAX_BINS (1ull << 22)
#define TFFT_FINISH1_MAX_IMAGES 4
struct MedianPlan { bool compact, finish1; int launches; };      // launches: kernels per launch_medians call
MedianPlan plan_medians(int PH, int PW, int n_images, const StatOpts& o);
hipError_t launch_medians(const float2* spec, int PH, int PW, size_t img_stride, int n_images, const StatBufs& b, const StatOpts& o, hipStream_t s);
// the statistics around a COLS_STAT step: bracket guess before it, select and settle after it; stat_tile_launches: their kernels
hipError_t launch_stat_guess(const float2* mini, int PH, int PW, int Ms, size_t mini_img_stride, int col0_packed, int n_images, const StatBufs& b,
                             const StatOpts& o, hipStream_t s);
hipError_t launch_stat_select(int PH, int n_images, const StatBufs& b, hipStream_t s);
hipError_t launch_stat_settle(const float2* spec, int PH, int PW, size_t img_stride, int n_images, const StatBufs& b, const StatOpts& o, hipStream_t s);
int stat_tile_launches(const StatOpts& o);
int collect_bracket_resident_blocks();
// only_flagged: nullptr, or one word per image -- images whose word is 0 are skipped
hipError_t launch_capacity(const float2* spec, const CapParams& P, int n_images, const float* med_dev,
                           unsigned* partial, unsigned long long* usable, hipStream_t s, const unsigned* only_flagged);
hipError_t launch_frame_expand(const uint8_t* header, const uint8_t* payload, uint64_t plen, int n_images, uint8_t* bits,
                               uint64_t stride, hipStream_t s);      // image i's bits at bits + i*stride
hipError_t launch_frame_majority(const uint8_t* bits, uint64_t plen, int n_images, uint8_t* header, uint8_t* payload,
                                 hipStream_t s);
hipError_t launch_stream_decode(const uint8_t* bits, uint64_t n_bins, uint64_t max_plen, int n_images, uint8_t* header, uint8_t* payload,
                                int* status, unsigned* plen, hipStream_t s);
hipError_t launch_export_full(const float2* spec, int PH, int PW, int PWout, float2* out, hipStream_t s);
// compute_cover_hash's low-frequency magnitudes in fp64 from the pixels (rowsum: H*3*region double2 of scratch)
hipError_t launch_lowfreq_f64(const uint8_t* rgb, int W, int H, int PW, int PH, int center, int region, double2* rowsum, double* out,
                              hipStream_t s);
// ... for n_images images of a batch (W*H*3 bytes apart): rowsum of image i at rowsum + i*rowsum_stride (double2), out at out + i*3*region^2;
// the same summation order as the single image, bit for bit
hipError_t launch_lowfreq_f64_batch(const uint8_t* rgb, int W, int H, int PW, int PH, int center, int region, int n_images, double2* rowsum,
                                    size_t rowsum_stride, double* out, hipStream_t s);

// ---- stego analysis
// annulus phase histograms of n_images resident spectra (img_stride apart): hist_out[(img*3 + plane)*nbins + bin], uint32
struct PhaseHistParams {
    CapParams cap;          // the annulus box, its exact radius bounds and img_stride (cap_params; thr / magmin unused)
    float t2[3];            // per plane: bins with |F|^2 < t2 are not counted (mag2_threshold(thr); -inf: no magnitude test)
    int log_bins;           // nbins = 1 << log_bins, 3..12
};
#define TFFT_PH_PARTIAL_WORDS 65536      // partial-histogram words per (image, plane) at most (blocks x nbins)
int phase_hist_blocks(const CapParams& cp, int log_bins, int n_images);      // partial = n_images*3*blocks*nbins words
hipError_t launch_phase_hist(const float2* spec, const PhaseHistParams& P, int n_images, unsigned* partial, uint32_t* hist_out, hipStream_t s);
// cover / stego quality of n_images image pairs (W*H*3 bytes apart): sse_out, ssim_out (or nullptr) per (image, plane);
// partials: n_images*3*quality_partials(W, H) of each kind
#define TFFT_QA_TX 64                    // window positions per tile (columns x rows)
#define TFFT_QA_TY 32
#define TFFT_QA_LDS_OFF 18656            // both images' bytes of a tile + halo, 3 planes: 2*3*(TY+10)*(TX+10), rounded up to 16
#define TFFT_QA_LDS (TFFT_QA_LDS_OFF + 5 * (TFFT_QA_TY + 10) * TFFT_QA_TX * 4)      // + the horizontal pass's five moments, fp32
#define TFFT_QA_C1 6.5025f               // (K1 L)^2, K1 = 0.01, L = 255
#define TFFT_QA_C2 58.5225f              // (K2 L)^2, K2 = 0.03
static_assert(TFFT_QA_LDS_OFF >= 2 * 3 * (TFFT_QA_TY + 10) * (TFFT_QA_TX + 10) && TFFT_QA_LDS_OFF % 16 == 0, "quality tile bytes");
struct QualityParams { int W, H; float g[11]; };      // g: the 11-tap Gaussian (sigma 1.5), normalised to sum 1
size_t quality_partials(int W, int H);
hipError_t launch_quality(const uint8_t* a, const uint8_t* b, const QualityParams& P, int n_images, unsigned long long* sse_part, double* ssim_part,
                          unsigned long long* sse_out, double* ssim_out, hipStream_t s);

// ---- robustness analysis: the channels a stego batch goes through, and the error counts of what is read back
// AWGN over a packed byte stream (in may equal out): byte j of the launch carries counter index0 + j of the noise sequence of `seed`
hipError_t launch_channel_awgn(const uint8_t* in, uint8_t* out, size_t n_bytes, uint64_t seed, uint64_t index0, float sigma, hipStream_t s);
// JPEG quantisation of n_images packed W x H RGB8 images (in may equal out): 8 x 8 blocks from (0, 0), 4:4:4, IJG-scaled Annex K tables
#define TFFT_JQ_COLS 256                 // pixel columns of one workgroup's strip of 8 image rows: 32 blocks, a thread per block row
#define TFFT_JQ_IN_PITCH 196             // dwords per staged input row: 3 + 768 + 3 bytes, and the 7-dword window of the last thread
#define TFFT_JQ_OUT_PITCH 194            // dwords per output row: one in front of the 192 of the strip and one behind (the store's byte shift)
#define TFFT_JQ_TR (32 * 3 * 8 * 9)      // floats of the transpose buffer: 32 blocks x 3 components x 8 rows of pitch 9
#define TFFT_JQ_LDS ((8 * TFFT_JQ_IN_PITCH + 8 * TFFT_JQ_OUT_PITCH + TFFT_JQ_TR + 128) * 4)
hipError_t launch_channel_jpeg(const uint8_t* in, uint8_t* out, int W, int H, int n_images, int quality, hipStream_t s);
// per image: raw bits (n_bins apart) against the Rep-3 / Rep-7 stream of its header (38 bytes) and payload (plen bytes), and the
// majority decode at that length against the bytes themselves: result[4*img + 0..2] = raw bit errors, header byte errors, payload byte
// errors (ADDED to what is there: the caller zeroes), result[4*img + 3] = status[img]
hipError_t launch_robust_count(const uint8_t* raw, uint64_t n_bins, const uint8_t* header, const uint8_t* payload, uint64_t plen,
                               const int* status, int n_images, uint32_t* result, hipStream_t s);

// ---- SPAM steganalysis features: counts[image][plane][dir][n^3] of the clamped difference triples, n = 2t + 1, t in 1..4
#define TFFT_SP_COLS 256                 // pixel columns of a workgroup's tile: 768 bytes, three per thread and row
#define TFFT_SP_ROWS 13                  // rows of the tile a workgroup counts per step; with the 3 rows of halo below them:
#define TFFT_SP_STAGE_ROWS 16
#define TFFT_SP_PITCH 198                // dwords per staged row: 3 (byte shift) + 3 * (3 + 256 + 3) bytes
int spam_bands(int W, int H, int t, int n_images, int* band_rows);      // workgroups per column tile and image, and the rows each owns
// zeroes counts (n_images * 12 n^3 words) and counts into it; n_images <= 65535
hipError_t launch_spam(const uint8_t* rgb, int W, int H, int n_images, int t, uint32_t* counts, hipStream_t s);

}  // namespace tfft
