/* turtlefft_hip.h -- C ABI of libturtlefft_hip.so, the MI355X (gfx950) replacement
 * for the 2-D-FFT phase-embedding hot path of rickenator/steganosaurus.
 *
 * The reference has no FFI layer: the path is reachable only through the
 * file-static functions of steganosaurus/src/steganosaur.cpp (cited S:<line>).
 * Each entry point below names the reference lines it replaces; INTEGRATION.md
 * shows the patch a maintainer of the reference would apply to do_embed /
 * do_extract to bind them.
 *
 * Conventions
 *   - every function returns TFFT_OK (0) or a negative tfft_status; nothing
 *     calls exit() and nothing throws across the boundary;
 *   - a context owns all device memory, its HIP stream(s) and twiddle tables;
 *     one context is used from one host thread at a time, distinct contexts
 *     (also on distinct devices) may be used concurrently;
 *   - "slot" = one resident image: its three half-spectra stay in HBM between
 *     calls (forward -> medians/capacity -> embed/read -> inverse), exactly the
 *     lifetime of FR/FG/FB/F3 in the reference (S:917-1100);
 *   - pointers are HOST pointers unless the function name ends in _dev, in
 *     which case they are device pointers valid on the context's device;
 *   - transforms use the reference's sign convention: forward kernel
 *     exp(+2*pi*i*nk/N) (S:347), inverse exp(-...) scaled 1/N per dimension
 *     (S:357); images are zero-padded to next_pow2 in each dimension (S:393-398)
 *     and the inverse crops back to W x H (S:399-403);
 *   - there is no CPU fallback: without a usable gfx950 device tfft_create
 *     fails with TFFT_E_NO_DEVICE.
 */
#ifndef TURTLEFFT_HIP_H
#define TURTLEFFT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TFFT_ABI_VERSION 1

typedef enum tfft_status {
    TFFT_OK = 0,
    TFFT_E_INVALID = -1,      /* bad argument (null pointer, slot out of range, size 0 ...) */
    TFFT_E_NO_DEVICE = -2,    /* no HIP device / not gfx950 / HIP runtime error at create */
    TFFT_E_TOO_LARGE = -3,    /* image larger than the context was created for, or > TFFT_MAX_DIM */
    TFFT_E_NOMEM = -4,        /* host or device allocation failed */
    TFFT_E_HIP = -5,          /* HIP runtime error during a launch/copy (see tfft_last_hip_error) */
    TFFT_E_STATE = -6,        /* slot holds no forward spectrum yet */
    TFFT_E_EXHAUSTED = -7,    /* walk: annulus exhausted (the reference would spin forever) */
    TFFT_E_BIN_RANGE = -8     /* a bin lies outside the padded grid or on an excluded axis */
} tfft_status;

#define TFFT_MAX_DIM 16384     /* largest padded width/height handled (rows of PW/2 complex fit in LDS) */

typedef struct tfft_ctx tfft_ctx;
typedef struct tfft_walk tfft_walk;

/* One embedding position, as produced by Turtle::advance_to_valid (S:778-804):
 * colour plane 0..2 and UN-shifted frequency indices on the padded grid. */
typedef struct tfft_bin {
    uint16_t x;        /* 0 .. PW-1 */
    uint16_t y;        /* 0 .. PH-1 */
    uint8_t plane;     /* 0=R 1=G 2=B */
    uint8_t rsv[3];    /* must be 0 */
} tfft_bin;

/* ------------------------------------------------------------------ context */
int tfft_abi_version(void);
const char* tfft_strerror(int status);

/* Allocates `n_slots` resident images of up to max_w x max_h pixels on HIP
 * device `device`.  Replaces the vectors of S:912-917 / S:1015. */
int tfft_create(int device, int max_w, int max_h, int n_slots, tfft_ctx** out);
int tfft_destroy(tfft_ctx* ctx);
/* Run all work of this context on an existing HIP stream (e.g. the framework's
 * current stream) instead of the context's own.  stream = hipStream_t. */
int tfft_set_stream(tfft_ctx* ctx, void* hip_stream);
int tfft_sync(tfft_ctx* ctx);
int tfft_last_hip_error(const tfft_ctx* ctx);
size_t tfft_device_bytes(const tfft_ctx* ctx);
/* Which kernels a launch over n_images images of w x h takes on this context (measurement / documentation aid):
 * info[0] = 1 when the column transform is one pass, else it is two steps of lengths 2^info[1] and 2^info[2];
 * info[3] = 1 when the row pass is fused with the adjacent column step (a 2-D transform is then two global passes:
 * always for images that pad to 2048 columns, for 4096 columns in launches of two or more images). */
int tfft_plan_info(const tfft_ctx* ctx, int w, int h, int n_images, int info[4]);

/* ------------------------------------------------------------- forward side
 * to_planes_u8 + apply_center + pad_to_fft + fft2d(forward) x3  (S:912-921,
 * S:1116-1123).  rgb = H*W*3 interleaved bytes.  Returns the padded size. */
int tfft_forward_rgb8(tfft_ctx* ctx, int slot, const uint8_t* rgb, int w, int h, int center, int* pw, int* ph);
int tfft_forward_rgb8_dev(tfft_ctx* ctx, int slot, const void* rgb_dev, int w, int h, int center, int* pw, int* ph);

/* median_abs x3 (S:922, S:404-409): element at sorted index P/2 of |F| over
 * the FULL padded plane (mirror bins counted).  Synchronises.
 * EXACT against the reference's fp64 spectrum (to ~1e-13 relative: two fp64 summation orders): the fp32 spectrum locates the
 * element, the handful of bins within 2e-6 of it are re-evaluated in fp64 from the pixels (tfft_exact.hip), and rank and value
 * are settled on those.  Needs the image of the last tfft_forward_rgb8[_dev] of the slot to be still in place (the _dev form
 * keeps the caller's pointer, like tfft_lowfreq_mag) and PW <= 8192; otherwise -- and with TFFT_EXACT_STATS=0 -- the order
 * statistic of the fp32 magnitudes is returned (2e-6 relative).  tfft_exact_info tells which. */
int tfft_medians(tfft_ctx* ctx, int slot, double med[3]);
/* bins per plane the last tfft_medians / tfft_capacity of this context re-evaluated in fp64 (0: the fp32 answer was returned) */
int tfft_exact_info(const tfft_ctx* ctx, int n_fp64[3]);

/* Diagnostic: how the last tfft_medians / batched median of `slot` was obtained, per plane:
 * 1 = sampled bracket + one verified pass (fast path), 0 = full three-level select (fallback). */
int tfft_median_path(tfft_ctx* ctx, int slot, int fast[3]);
/* Diagnostics of the batched embeds.  tfft_batch_medians: the fp32 medians |F| the statistics of the last batched embed left for the image
 * in `slot` (image i of a call's last chunk sits in slot i; no fp64 settling, nothing recomputed).  Synchronises.
 * tfft_embed_plan_info: the launch sequence the last chunk of the last batched embed took -- info[0] = 1: delta embedding; info[1]: the
 * statistics (0 none, 1 inside the last forward column step, 2 medians + capacity in one sequence, 3 separate passes); info[2] = 1: that
 * step also embedded and ran the first inverse column step (one launch for the pair); info[3] = 1: statistics on the side stream. */
int tfft_batch_medians(tfft_ctx* ctx, int slot, float med[3]);
int tfft_embed_plan_info(const tfft_ctx* ctx, int info[4]);

/* count_plane (S:998-1008): sum over planes of floor(c/2), c = bins in the
 * annulus [rmin,rmax]*min(PH,PW), off the axes, |F| >= thr[plane].  Synchronises.
 * EXACT like tfft_medians (same conditions): bins within 1e-3 of thr are settled on their fp64 magnitudes, so with
 * thr = magmin * tfft_medians() the count is the reference's integer.  The batched pipelines' usable_out is the count on the
 * fp32 planes (observed 0-1 off, bound 2: a bin within fp32 rounding of the threshold) unless tfft_set_batch_exact asks for this
 * integer there too, see DESIGN.md sections 2 and 11. */
int tfft_capacity(tfft_ctx* ctx, int slot, double rmin, double rmax, const double thr[3], uint64_t* usable);

/* compute_cover_hash's magnitudes (S:428-436): |F[y][x]| for y,x < region (<= 8) of
 * each plane, out = 3*region*region doubles in plane, y, x order.  Evaluated in fp64
 * straight from the image the slot's last tfft_forward_rgb8[_dev] call read (for the
 * _dev variant that buffer must still be alive): 192 inner products, no transform,
 * so the reference's quantiser floor(log(1+mag)/2) (S:433) sees its own values to
 * ~1e-13 and the 32-byte cover hash is the reference's.  TFFT_E_STATE after a batch
 * call (no single image belongs to the slot: tfft_lowfreq_mag_batch_dev serves batches).  Synchronises. */
int tfft_lowfreq_mag(tfft_ctx* ctx, int slot, int region, double* out);

/* ------------------------------------------------------------- embed / read
 * The embed loop body, write_bit_on_bin (S:712-732), over a materialised bin
 * list: F[y][x] = polar(max(1e-12,|F|), (bit ? +a : -a) + jitter[i]) and the
 * Hermitian mirror = conj.  a = alpha, or alpha*clamp(|F|/med[plane],0.5,2)
 * when `adaptive` (S:704-710).  jitter may be NULL (all zero).  Bins of one
 * list must be distinct with distinct mirrors (the walk guarantees it). */
int tfft_embed_bins(tfft_ctx* ctx, int slot, const tfft_bin* bins, const uint8_t* bits, const float* jitter,
                    uint64_t n, double alpha, int adaptive, const double med[3]);
int tfft_embed_bins_dev(tfft_ctx* ctx, int slot, const void* bins_dev, const void* bits_dev, const void* jitter_dev,
                        uint64_t n, double alpha, int adaptive, const double med[3]);

/* read_bit_from_bin (S:734-746) over a bin list: bits_out[i] in {0,1}.  May be
 * called repeatedly on a resident spectrum (912 header bits, then the payload:
 * S:1223-1264).  The host variant synchronises. */
int tfft_read_bins(tfft_ctx* ctx, int slot, const tfft_bin* bins, const float* jitter, uint64_t n, double alpha,
                   int adaptive, const double med[3], uint8_t* bits_out);
int tfft_read_bins_dev(tfft_ctx* ctx, int slot, const void* bins_dev, const void* jitter_dev, uint64_t n,
                       double alpha, int adaptive, const double med[3], void* bits_out_dev);

/* ------------------------------------------------------------- inverse side
 * fft2d(inverse) x3 + ifft_crop + apply_center + from_planes_u8 (S:1100-1103):
 * real part, round half away from zero, clamp to 0..255, interleave.  The
 * slot's spectrum is consumed.  The host variant synchronises. */
int tfft_inverse_rgb8(tfft_ctx* ctx, int slot, uint8_t* rgb_out);
int tfft_inverse_rgb8_dev(tfft_ctx* ctx, int slot, void* rgb_out_dev);

/* Parity/debug export: the FULL padded spectra, 3*PH*PW interleaved (re,im)
 * floats, mirror half reconstructed by Hermitian symmetry.  Synchronises. */
int tfft_download_spectrum(tfft_ctx* ctx, int slot, float* out);

/* ---------------------------------------------------- fp64 audit transform
 *   The reference's fft2d (S:341-366) evaluated in double on the
 * device, operation by operation: bit reversal, radix-2 DIT stages, stage
 * twiddles by the recurrence w *= wlen, no FMA contraction, rows then columns,
 * inverse divided by n per dimension.  Its output equals the CPU reference bit
 * for bit (checked against the oracle); it exists to measure the fp32 product
 * path against the reference's arithmetic at sizes where the CPU takes minutes.
 * Slow by design (one global pass per stage).  Host buffers; synchronises.
 *   tfft_audit_fft2d_f64        in place on n_planes planes of ph x pw interleaved
 *                               (re,im) doubles; ph, pw powers of two.
 *   tfft_audit_forward_rgb8_f64 to_planes_u8 + apply_center + pad_to_fft + fft2d
 *                               forward x3 (S:912-921): out = 3*PH*PW*2 doubles. */
int tfft_audit_fft2d_f64(tfft_ctx* ctx, double* planes, int n_planes, int ph, int pw, int inverse);
int tfft_audit_forward_rgb8_f64(tfft_ctx* ctx, const uint8_t* rgb, int w, int h, int center, double* out);

/* ------------------------------------------------------------------ batches
 * n independent images of identical size sharing ONE bin list (the walk does
 * not depend on image content: S:797-799).  Images are processed in chunks of
 * n_slots; every pipeline stage of a chunk is ONE kernel launch over all its
 * images, on the context's stream.  All pointers are device pointers;
 * image i is at rgb + i*w*h*3, its bits at bits + i*n_bits.
 *   embed  : forward -> [medians+capacity when usable_out != NULL] -> embed -> inverse
 *   extract: forward -> read
 * usable_out (device, n uint64) receives each image's capacity so the caller
 * can raise "Message too large" (S:1009-1012) without a sync per image: the count
 * on the fp32 planes (0-2 off the reference's integer), or with tfft_set_batch_exact
 * the reference's integer itself.
 * The embed pipeline uses the linearity of S:1099-1103: stego = clamp(round(cover +
 * IFFT(F' - F))), F' - F being zero but at the bins of the list -- the modified spectrum
 * is never written, the cover buffer is read once more by the last kernel (in-place
 * embedding, rgb_out_dev == rgb_dev, is allowed).  Same image as inverting F' in exact
 * arithmetic; in fp32 it is 1 LSB away from what tfft_embed_bins + tfft_inverse_rgb8
 * return on a few pixels per million (both within 1 LSB of the fp64 reference). */
int tfft_embed_batch_dev(tfft_ctx* ctx, int n_images, const void* rgb_dev, int w, int h, int center,
                         const void* bins_dev, const void* bits_dev, uint64_t n_bits, double alpha,
                         double rmin, double rmax, double magmin, void* usable_out_dev, void* rgb_out_dev);
int tfft_extract_batch_dev(tfft_ctx* ctx, int n_images, const void* rgb_dev, int w, int h, int center,
                           const void* bins_dev, uint64_t n_bits, double alpha, void* bits_out_dev);

/* Stream framing on the device.  expand: for each of n_images, the 38-byte header and
 * payload_len bytes of (ciphertext || tag) become the one-byte-per-bit stream Rep-3(header) || Rep-7(payload),
 * MSB first -- bits_from_bytes + rep3/rep7_encode (S:455-467, S:494-500, S:986-995).  majority: the inverse,
 * rep3/rep7_decode + bytes_from_bits (S:447-454, S:468-474, S:501-508) on 912 + 56*payload_len raw bits per
 * image.  header/payload arrays are packed per image (38 and payload_len bytes apart). */
int tfft_frame_expand_dev(tfft_ctx* ctx, int n_images, const void* header_dev, const void* payload_dev, uint64_t payload_len,
                          void* bits_out_dev);
int tfft_frame_majority_dev(tfft_ctx* ctx, int n_images, const void* bits_dev, uint64_t payload_len, void* header_out_dev,
                            void* payload_out_dev);

/* The same two pipelines on PACKED BYTES, i.e. what do_embed / do_extract do around the walk (f-3 inside the
 * pipelines: only 38 + payload_len bytes per image would have to cross PCIe):
 *   embed  : header (38 B) and payload (ciphertext || tag, payload_len bytes) per image -> Rep-3 / Rep-7 stream
 *            on the device (S:986-995) -> the first 912 + 56*payload_len positions of the caller's walk (n_bins
 *            of them, n_bins >= that, else TFFT_E_INVALID) -> inverse.
 *   extract: forward -> the raw bit of EVERY position of the caller's walk, read in the one pass that has the
 *            spectrum on chip -> Rep-3 majority of the first 912 -> header bytes -> magic, version, clen ->
 *            Rep-7 majority of the next 56*(clen+16) bits of the same walk (S:1223-1264).  The length comes out
 *            of the image, not from the caller.
 *            status_out[i] (int32) = clen >= 0, or -1 "Magic not found.", -2 "Unsupported version" (header byte 4
 *            holds it), -3 the walk (n_bins) or the payload buffer (max_payload_len) is too short for what the
 *            header announces (where the reference keeps walking, S:1260-1264).
 *            header_out: 38 bytes per image (always written; the AAD of S:1299-1301).  payload_out: clen+16 bytes
 *            per image at stride max_payload_len.  raw_bits_out (optional): the n_bins raw bits per image.
 * n_bins is also the length a bit index (tfft_set_bit_index) must have been set for. */
int tfft_embed_stream_batch_dev(tfft_ctx* ctx, int n_images, const void* rgb_dev, int w, int h, int center,
                                const void* bins_dev, uint64_t n_bins, const void* header_dev, const void* payload_dev,
                                uint64_t payload_len, double alpha, double rmin, double rmax, double magmin,
                                void* usable_out_dev, void* rgb_out_dev);
int tfft_extract_stream_batch_dev(tfft_ctx* ctx, int n_images, const void* rgb_dev, int w, int h, int center,
                                  const void* bins_dev, uint64_t n_bins, double alpha, void* header_out_dev,
                                  void* payload_out_dev, uint64_t max_payload_len, void* status_out_dev,
                                  void* raw_bits_out_dev);

/* The same two pipelines for HOST buffers (images packed back to back, one byte per bit): the slots
 * are split into two halves and three HIP streams overlap the PCIe copy-in of the next half-batch,
 * the kernels of the current one and the copy-out of the previous one.  The
 * transfers overlap only when the host buffers are page-locked: tfft_host_alloc / tfft_host_free, or
 * any pinned allocation.  Both calls return after the last result has landed. */
int tfft_embed_batch(tfft_ctx* ctx, int n_images, const uint8_t* rgb, int w, int h, int center, const tfft_bin* bins,
                     const uint8_t* bits, uint64_t n_bits, double alpha, double rmin, double rmax, double magmin,
                     uint64_t* usable_out /* or NULL */, uint8_t* rgb_out);
int tfft_extract_batch(tfft_ctx* ctx, int n_images, const uint8_t* rgb, int w, int h, int center, const tfft_bin* bins,
                       uint64_t n_bits, double alpha, uint8_t* bits_out);
/* ... and on packed bytes: 38 + payload_len bytes per image go in, 38 + clen + 16 bytes and a status word come out, instead of
 * one byte per stream bit (the framing and the two-phase decode run on the device inside the same three-stream pipeline; semantics
 * as tfft_*_stream_batch_dev; raw_bits_out may be NULL). */
int tfft_embed_stream_batch(tfft_ctx* ctx, int n_images, const uint8_t* rgb, int w, int h, int center, const tfft_bin* bins,
                            uint64_t n_bins, const uint8_t* header, const uint8_t* payload, uint64_t payload_len, double alpha,
                            double rmin, double rmax, double magmin, uint64_t* usable_out /* or NULL */, uint8_t* rgb_out);
int tfft_extract_stream_batch(tfft_ctx* ctx, int n_images, const uint8_t* rgb, int w, int h, int center, const tfft_bin* bins,
                              uint64_t n_bins, double alpha, uint8_t* header_out, uint8_t* payload_out, uint64_t max_payload_len,
                              int32_t* status_out, uint8_t* raw_bits_out /* or NULL */);
void* tfft_host_alloc(size_t bytes);
void tfft_host_free(void* p);

/* ------------------------------------------------------ one walk per image
 * The stream pipelines above for batches whose images do NOT share a walk: images with their own passphrase or key, and
 * --cover_dependent_path 1 (path_key = SHA256(pass | key || cover_hash), S:1020-1039), where every cover has its own walk even under one
 * passphrase.  Semantics as tfft_*_stream_batch[_dev], image by image, with these differences:
 *   bins     : n_images walks of n_bins positions each, image i's at bins + i*n_bins, in WALK (= stream) order (not sorted: there is no
 *              bit index; every entry's stream position is its place in the image's own list);
 *   jitter   : n_images*n_bins floats in the same layout (tfft_walk_jitter of each image's own plane keys), or NULL (no jitter);
 *   adaptive : adaptive alpha (S:704-710) with each image's own medians, the rules of tfft_set_phase_options (extraction: |alpha| >= pi/2
 *              gives TFFT_E_INVALID);
 *   the context's shared-list state does not mix with these calls: with a bit index (tfft_set_bit_index) or a phase-option jitter array
 *   (tfft_set_phase_options) set they return TFFT_E_STATE (the context's adaptive flag is ignored: `adaptive` rules);
 *   a bin outside the grid or on an excluded axis in any image's list gives TFFT_E_BIN_RANGE: the _dev forms synchronise with the
 *   context's stream at their end to report it;
 *   the buckets of the tile-resident kernels are built from the lists on every call; no launch sequence is captured into or replayed
 *   from the graph cache (TFFT_GRAPHS), and tfft_bins_register_dev does not apply;
 *   n_slots * n_bins must stay below 2^32 (else TFFT_E_TOO_LARGE).
 * The host forms run the three-stream pipeline of tfft_*_stream_batch: lists and jitter travel per part of the ring with the images
 * (8 + 4 bytes per position and image).  Crypto stays with the caller (libtfhost / the CLI): HKDF, the cover-hash quantiser. */
int tfft_embed_stream_batch_walks_dev(tfft_ctx* ctx, int n_images, const void* rgb_dev, int w, int h, int center,
                                      const void* bins_dev, const void* jitter_dev, uint64_t n_bins, int adaptive,
                                      const void* header_dev, const void* payload_dev, uint64_t payload_len,
                                      double alpha, double rmin, double rmax, double magmin, void* usable_out_dev, void* rgb_out_dev);
int tfft_extract_stream_batch_walks_dev(tfft_ctx* ctx, int n_images, const void* rgb_dev, int w, int h, int center,
                                        const void* bins_dev, const void* jitter_dev, uint64_t n_bins, int adaptive, double alpha,
                                        void* header_out_dev, void* payload_out_dev, uint64_t max_payload_len, void* status_out_dev,
                                        void* raw_bits_out_dev);
int tfft_embed_stream_batch_walks(tfft_ctx* ctx, int n_images, const uint8_t* rgb, int w, int h, int center, const tfft_bin* bins,
                                  const float* jitter, uint64_t n_bins, int adaptive, const uint8_t* header, const uint8_t* payload,
                                  uint64_t payload_len, double alpha, double rmin, double rmax, double magmin,
                                  uint64_t* usable_out /* or NULL */, uint8_t* rgb_out);
int tfft_extract_stream_batch_walks(tfft_ctx* ctx, int n_images, const uint8_t* rgb, int w, int h, int center, const tfft_bin* bins,
                                    const float* jitter, uint64_t n_bins, int adaptive, double alpha, uint8_t* header_out,
                                    uint8_t* payload_out, uint64_t max_payload_len, int32_t* status_out,
                                    uint8_t* raw_bits_out /* or NULL */);
/* ------------------------------------------------------ fitted embed: stego of non-power-of-two covers that reads back
 * The embed changes bins of the zero-padded next_pow2 spectrum and the inverse crops back to W x H: on a cover whose sides are not
 * powers of two the crop loses much of every change and the stego does not read back (in the reference either).  This separate,
 * non-default mode fits the stego instead, for 0 < alpha < pi/2, where the reader's decision is the side of a line (bit 1 <=>
 * Im(F e^{-ij}) >= 0): after the walks embed, every chunk alternates a forward transform of the rounded stego, a correction of the deltas
 * of the bins that read on the wrong side of a margin mu = max(margin * |F0| * sin(alpha_k), 3 * sqrt(W*H/24)) and the delta inverse,
 * until every image reads every stream bit right with at least mu/2 to spare or max_iters corrections are done.
 * The stego is an ordinary one: the unmodified extractors (tfft_extract_stream_batch_walks*, the reference CLI) read it.
 * Semantics, state rules, errors and limits of tfft_embed_stream_batch_walks[_dev], and:
 *   alpha must lie in (0, pi/2), max_iters >= 0 and margin > 0 (default 0.5), else TFFT_E_INVALID;
 *   iters_out (int32 per image, or NULL): corrections applied to the image, -1 if it did not converge within max_iters (not an error:
 *   the stego is written);  wrong_out (uint32 per image, or NULL): stream bits that read wrong from the returned bytes;
 *   max_iters = 0 returns the bytes and usable_out of tfft_embed_stream_batch_walks[_dev] (and the counts of those bytes);
 *   rgb_out may be rgb (each chunk's covers are copied first); the call synchronises once per iteration to read the counts.
 * The host form stages one chunk of n_slots images at a time. */
int tfft_embed_stream_batch_fit_dev(tfft_ctx* ctx, int n_images, const void* rgb_dev, int w, int h, int center,
                                    const void* bins_dev, const void* jitter_dev, uint64_t n_bins, int adaptive,
                                    const void* header_dev, const void* payload_dev, uint64_t payload_len,
                                    double alpha, double rmin, double rmax, double magmin, int max_iters, double margin,
                                    void* usable_out_dev, void* iters_out_dev, void* wrong_out_dev, void* rgb_out_dev);
int tfft_embed_stream_batch_fit(tfft_ctx* ctx, int n_images, const uint8_t* rgb, int w, int h, int center, const tfft_bin* bins,
                                const float* jitter, uint64_t n_bins, int adaptive, const uint8_t* header, const uint8_t* payload,
                                uint64_t payload_len, double alpha, double rmin, double rmax, double magmin, int max_iters, double margin,
                                uint64_t* usable_out /* or NULL */, int32_t* iters_out /* or NULL */, uint32_t* wrong_out /* or NULL */,
                                uint8_t* rgb_out);
/* compute_cover_hash's magnitudes (S:428-436) for the n_images images of a batch (device pointers, image i at rgb + i*w*h*3):
 * out = n_images*3*region*region doubles, image i's at out + i*3*region*region -- the same values, bit for bit, as tfft_lowfreq_mag on
 * each image alone (same kernels, same summation order).  Needs no forward call and leaves the slots alone; does not synchronise.
 * The quantiser + SHA-256 of the hash stay with the caller (libtfhost: tfh_cover_hash_from_mags). */
int tfft_lowfreq_mag_batch_dev(tfft_ctx* ctx, int n_images, const void* rgb_dev, int w, int h, int center, int region, void* out_dev);

/* ------------------------------------------------------------ stego analysis
 * What a stego batch gives away, measured on the device (the phase-histogram detector and the PSNR / SSIM of the reference's security
 * analysis).  Per image and plane: a histogram of the phases of the annulus bins of the image's padded spectrum -- the bins count_plane
 * (S:998-1008) counts: full-plane unshifted (y, x), y != 0, x != 0, 2y != PH, 2x != PW, rmin*mn <= hypot(y, x) <= rmax*mn, and
 * |F| >= thr[plane] under the capacity kernels' fp32 test (thr == NULL: no magnitude test).
 * theta = atan2(Im F, Re F) of the full-plane coefficient in the reference's sign convention (the angle read_bit_from_bin, S:736, takes);
 * for x > PW/2 that is minus the angle of the stored mirror.  bin = floor((theta + pi) * n_hist_bins / (2 pi)) mod n_hist_bins (theta = +-pi
 * both land in bin 0).  hist_out: uint32, image i plane p at (i*3 + p)*n_hist_bins.  n_hist_bins: a power of two in [8, 4096].
 * Needs no bin list or medians, and ignores the bit index, the registered list and the phase options.  Overwrites the slots' spectra, as a
 * batch call does (tfft_lowfreq_mag then gives TFFT_E_STATE).  The _dev form does not synchronise (but for growing its scratch on first
 * use); the host form stages one chunk of n_slots images at a time and synchronises. */
int tfft_phase_hist_batch_dev(tfft_ctx* ctx, int n_images, const void* rgb_dev, int w, int h, int center, double rmin, double rmax,
                              const double thr[3] /* or NULL */, int n_hist_bins, void* hist_out_dev);
int tfft_phase_hist_batch(tfft_ctx* ctx, int n_images, const uint8_t* rgb, int w, int h, int center, double rmin, double rmax,
                          const double thr[3] /* or NULL */, int n_hist_bins, uint32_t* hist_out);
/* a, b: n_images RGB8 images of w x h (image i at + i*w*h*3).  sse_out: uint64 per image and plane, sum of (a - b)^2, exact.
 * ssim_out (double per image and plane, or NULL): mean SSIM of the plane (Wang et al. 2004): 11 x 11 Gaussian window, sigma 1.5,
 * normalised to sum 1; K1 = 0.01, K2 = 0.03, L = 255; population moments (E[x^2] - mu^2, evaluated on pixel - 128 in fp32, the window means
 * added in fp64 in a fixed order); mean over the (W-10)(H-10) windows that lie inside the image; exactly 1.0 for a plane whose SSE is 0.
 * ssim_out with w < 11 or h < 11: TFFT_E_INVALID; w > max_w or h > max_h: TFFT_E_TOO_LARGE.  Leaves the slots alone (spectra and
 * image buffers: tfft_medians, tfft_capacity and tfft_lowfreq_mag of a resident image answer as before the call).
 * Deterministic: repeated calls return identical bytes.  PSNR = 10 log10(255^2 W H / SSE) per plane, +inf when SSE = 0 (the caller's).
 * The host form stages chunks in buffers of its own and synchronises. */
int tfft_quality_batch_dev(tfft_ctx* ctx, int n_images, const void* a_dev, const void* b_dev, int w, int h,
                           void* sse_out_dev, void* ssim_out_dev /* or NULL */);
int tfft_quality_batch(tfft_ctx* ctx, int n_images, const uint8_t* a, const uint8_t* b, int w, int h,
                       uint64_t* sse_out, double* ssim_out /* or NULL */);

/* ------------------------------------------------------------ robustness analysis
 * How much noise or recompression a stego batch survives, measured on the device: a channel attacks the images, the stream extractor reads them,
 * and the errors are counted against what was embedded (the "BER vs AWGN/JPEG" tests of the reference's roadmap).
 * A channel: kind 0 none (a copy); kind 1 AWGN, param = sigma in grey levels (>= 0, finite), seed used; kind 2 JPEG quantisation, param =
 * quality, an integer 1..100.  Images are packed RGB8, image i at + i*w*h*3; rgb_out may be rgb (in place).  first_image is the index of
 * image 0 in the caller's numbering: the bytes do not depend on how a batch is cut into calls, and repeated calls return identical bytes.
 *   AWGN, for image i (counted from first_image) and byte p = (y*w + x)*3 + c:  k = seed + 0x9E3779B97F4A7C15 * (i*w*h*3 + p) mod 2^64,
 *        z = splitmix64(k), u1 = ((z >> 40) + 0.5) / 2^24, u2 = (((z >> 16) & 0xFFFFFF) + 0.5) / 2^24, g = sqrt(-2 ln u1) cos(2 pi u2),
 *        out = clamp(rint(pixel + sigma*g), 0, 255), evaluated in fp32 (within 1e-4 max(1, sigma) of the fp64 value before rounding).
 *   JPEG quantisation: the lossy part of baseline JPEG, not its file format.  JFIF full-range BT.601 to Y - 128, Cb, Cr in floating point;
 *        4:4:4; 8 x 8 blocks from (0, 0), the right and bottom edge blocks completed by repeating the last column / row; orthonormal 2-D
 *        DCT-II; the Annex K luminance table for Y and chrominance table for Cb / Cr in natural order, scaled the IJG way (s = 5000 div Q for
 *        Q < 50, else 200 - 2Q; q = clamp((base*s + 50) div 100, 1, 255)); level = rint(c/q), c' = level*q; inverse DCT, Y + 128, inverse colour
 *        transform, clamp(rint(.), 0, 255).  Only the w x h pixels are written.
 *        Left out: chroma subsampling, the decoder's rounding of YCbCr to 8 bits, and entropy coding (lossless).  None changes the error
 *        mechanism that matters to a phase embedding, which is the quantisation of the coefficients.
 * Invalid kind, sigma < 0 or not finite, quality outside 1..100 or not an integer: TFFT_E_INVALID; w > max_w or h > max_h: TFFT_E_TOO_LARGE.
 * The calls leave the slots alone (like tfft_quality_batch).  The _dev form does not synchronise; the host form stages one chunk of n_slots
 * images at a time in the analysis scratch and synchronises. */
typedef struct tfft_channel { int32_t kind; float param; uint64_t seed; } tfft_channel;
int tfft_channel_batch_dev(tfft_ctx* ctx, int n_images, const void* rgb_dev, int w, int h, const tfft_channel* ch /* host */,
                           uint64_t first_image, void* rgb_out_dev);
int tfft_channel_batch(tfft_ctx* ctx, int n_images, const uint8_t* rgb, int w, int h, const tfft_channel* ch, uint64_t first_image,
                       uint8_t* rgb_out);
/* For every channel k and image i, result[(k*n_images + i)*4 ..] = {raw_bit_errors, header_byte_errors, payload_byte_errors, (uint32)status}
 * of the stego images read back after channel k, exactly as this sequence of calls on the same context gives them:
 *   1. tfft_channel_batch_dev(stego, channels[k], first_image) -> the attacked batch;
 *   2. tfft_extract_stream_batch_dev(attacked, bins, n_bins, alpha, ..., max_payload_len = payload_len, raw_bits_out) -> raw bits and status
 *      (clen, or -1 / -2 / -3); it honours the bit index, the registered list and tfft_set_phase_options as that call does;
 *   3. raw_bit_errors = Hamming distance of the first 912 + 56*payload_len raw bits to tfft_frame_expand_dev(header, payload, payload_len);
 *   4. header_byte_errors / payload_byte_errors = bytes of tfft_frame_majority_dev(raw bits, payload_len) that differ from the given header
 *      (38 bytes per image) and payload (payload_len bytes per image): a decode at the KNOWN length, so the error rate after the
 *      repetition code stays measurable when the header is lost.
 * n_bins >= 912 + 56*payload_len and n_channels >= 1, else TFFT_E_INVALID; otherwise the errors of the calls above.  Works chunk by chunk
 * (n_slots images, every channel in turn) and keeps one attacked copy of a chunk in the analysis scratch (grown on demand); stego_dev is never
 * written.  Results do not depend on n_slots, and repeated calls return the same.  The slots are left as by an extract batch call.  The _dev
 * form does not synchronise (but for growing the scratch); the host form stages chunk by chunk like tfft_phase_hist_batch and synchronises.
 * One list for all images: there is no _walks form. */
int tfft_robustness_batch_dev(tfft_ctx* ctx, int n_images, const void* stego_dev, int w, int h, int center,
                              const void* bins_dev, uint64_t n_bins, double alpha,
                              const void* header_dev, const void* payload_dev, uint64_t payload_len,
                              const tfft_channel* channels /* host */, int n_channels, uint64_t first_image,
                              void* result_out_dev /* uint32 [n_channels][n_images][4] */);
int tfft_robustness_batch(tfft_ctx* ctx, int n_images, const uint8_t* stego, int w, int h, int center,
                          const tfft_bin* bins, uint64_t n_bins, double alpha,
                          const uint8_t* header, const uint8_t* payload, uint64_t payload_len,
                          const tfft_channel* channels, int n_channels, uint64_t first_image, uint32_t* result_out);

/* ------------------------------------------------------------ blind steganalysis features
 * SPAM (Pevny, Bas, Fridrich 2010), second order: co-occurrence counts of clamped differences of neighbouring pixels, the features of a
 * spatial-domain steganalyser that knows nothing of the embedding.  Pure integer arithmetic on the pixels.
 * For one plane I of a packed RGB8 image of w x h, a truncation t in 1..4 and n = 2t + 1, four directions d = (dy, dx) are counted, in
 * this order: 0 right (0, 1), 1 down (1, 0), 2 down-right (1, 1), 3 down-left (1, -1).  For every pixel p = (y, x) with p + 3d inside the
 * image:
 *     e_k = clamp(I[p + (k-1)d] - I[p + kd], -t, t)   k = 1, 2, 3
 *     idx = ((e1 + t) n + (e2 + t)) n + (e3 + t)
 *     counts[image][plane][dir][idx] += 1
 * counts_out: uint32 [n_images][3][4][n^3] (686 * 6 words per image at t = 3).  Every entry is written; a direction with no triple (w < 4
 * or h < 4) is all zeros; direction d sums to max(0, h - 3|dy|) * max(0, w - 3|dx|).  The four opposite directions are not counted: they
 * are an index permutation, C_{-d}[a, b, c] = C_d[-c, -b, -a] (steganosaurus_amd/analysis.py: spam_features applies it and normalises as
 * the released extractor does, 2 n^3 features per plane).
 * Images are packed, image i at + i*w*h*3; only those n_images*w*h*3 bytes are read.  t outside 1..4, n_images < 1, w or h < 1:
 * TFFT_E_INVALID; w > max_w or h > max_h: TFFT_E_TOO_LARGE.  The calls leave the slots alone (like tfft_quality_batch): spectra, image
 * buffers, tfft_medians, tfft_capacity and tfft_lowfreq_mag of a resident image are as before.  Results do not depend on n_slots, and
 * repeated calls return identical bytes.  The _dev form does not synchronise (it needs no scratch); the host form stages one chunk of
 * n_slots images at a time in the analysis scratch and synchronises. */
int tfft_spam_batch_dev(tfft_ctx* ctx, int n_images, const void* rgb_dev, int w, int h, int t, void* counts_out_dev);
int tfft_spam_batch(tfft_ctx* ctx, int n_images, const uint8_t* rgb, int w, int h, int t, uint32_t* counts_out);

/* --------------------------------------------------------- keyed walk (HOST)
 * KS + Turtle + the density gate (S:665-695, S:749-810, S:1076-1081): a
 * resumable generator of embedding positions.  Pure host code, no device.
 * key_walk = first 32 bytes of HKDF-Expand(path_key, "turtle_keys") (S:1054-1058).
 * tfft_walk_next appends the next n positions; *skipped (optional) is
 * incremented by the density-rejected bins.  Returns TFFT_E_EXHAUSTED instead
 * of spinning when no acceptable bin is left. */
int tfft_walk_create(const uint8_t key_walk[32], int ph, int pw, double rmin, double rmax, double density,
                     tfft_walk** out);
int tfft_walk_next(tfft_walk* w, uint64_t n, tfft_bin* out, uint64_t* skipped);
int tfft_walk_start(const tfft_walk* w, int* plane, int* y, int* x);
uint32_t tfft_walk_ks_blocks(const tfft_walk* w);
int tfft_walk_destroy(tfft_walk* w);
/* KS::jitter (S:690-694) for a materialised list: out[i] = jitter drawn from
 * the plane's own keystream (keys_rgb = 3*32 bytes key_r|key_g|key_b) in list
 * order; two bytes are consumed per bin even when max_jitter == 0 (S:719). */
int tfft_walk_jitter(const uint8_t keys_rgb[96], const tfft_bin* bins, uint64_t n, double max_jitter, float* out);
/* n walks at once, for the per-image batch calls: keys = n*128 bytes, image i's walk key and R, G, B jitter keys at keys + 128*i
 * (key_walk | key_r | key_g | key_b, S:1054-1063).  bins_out (n*n_bins) and jitter_out (n*n_bins floats, or NULL) receive what
 * tfft_walk_create + tfft_walk_next(n_bins) + tfft_walk_jitter give for each key, bit for bit; status_out[i] = TFFT_OK or
 * TFFT_E_EXHAUSTED (that image's remaining positions and jitter are zero).  The walks run on up to n_threads threads (the caller sizes
 * the pool).  Returns TFFT_OK, or the first failing image's status. */
int tfft_walks_build(int n, const uint8_t* keys, int ph, int pw, double rmin, double rmax, double density, double max_jitter,
                     uint64_t n_bins, int n_threads, tfft_bin* bins_out, float* jitter_out, int32_t* status_out);

/* ------------------------------------------------------- bin visiting order
 * (new; no counterpart in the reference, whose loop S:1074-1097 visits the
 * bins in walk order because it materialises them one at a time.)  The walk
 * is a pseudo-random tour, so in walk order every bin is its own DRAM row
 * activation.  The result of embed/read does not depend on the order in which
 * distinct bins are visited (the walk never yields a bin or its mirror twice,
 * S:793-809), so the kernels may visit them in address order:
 *   tfft_bins_sort   (host) sorts `bins` in place by (plane, y, x) and writes
 *                    bit_index[i] = the position bins[i] had in the walk, i.e.
 *                    the stream bit it carries.  Compute jitter (tfft_walk_jitter)
 *                    BEFORE sorting: jitter stays indexed by stream bit.
 *   tfft_set_bit_index  hands that index (host array; copied to the device) to
 *                    the context.  From then on every embed/read/batch call on
 *                    it reads bits[bit_index[i]] / jitter[bit_index[i]] and
 *                    writes bits_out[bit_index[i]] for bins[i]; `bits`,
 *                    `jitter` and `bits_out` keep their stream order, so the
 *                    caller-visible results are identical to the unsorted call.
 *                    The index must be a permutation of 0..n-1 (else
 *                    TFFT_E_INVALID) and calls with a different n fail with
 *                    TFFT_E_STATE until it is cleared with (ctx, NULL, 0). */
int tfft_bins_sort(tfft_bin* bins, uint32_t* bit_index, uint64_t n);
/* Optional promise: the n bins at device pointer bins_dev will not change until they are registered again (or with NULL).  The
 * batch extraction calls that are handed exactly this list then keep what they derive from it -- the per-tile buckets of the
 * tile-resident read, the highest row the list touches -- instead of rebuilding it on every call (5 small launches, ~50 us per
 * 32 x 1080p call).  Results are identical either way; tfft_set_bit_index drops what was kept.  The batched EMBED calls use the
 * same cache (their delta form buckets the list too).  It is keyed on address and length: after rewriting the list in place, register
 * it again.  Bins outside the grid are reported (TFFT_E_BIN_RANGE) by every call on the registered list, not only the first. */
int tfft_bins_register_dev(tfft_ctx* ctx, const void* bins_dev, uint64_t n);
int tfft_set_bit_index(tfft_ctx* ctx, const uint32_t* bit_index, uint64_t n);

/* Phase options of the BATCHED calls (tfft_*_batch[_dev], tfft_*_stream_batch[_dev], tfp_*), the --jitter and --adaptive_alpha of
 * the reference CLI (S:690-694, S:704-710, S:719):
 *   jitter: n floats in STREAM order (tfft_walk_jitter, computed before tfft_bins_sort), copied to the device, or NULL.  Every image
 *           of a batch shares it, as it shares the bin list.  Calls with another n_bits / n_bins fail with TFFT_E_STATE while a jitter
 *           array is set.
 *   adaptive_alpha: a = alpha*clamp(|F|/med,0.5,2) with each image's own medians (the fp32 order statistic of the batch path, computed
 *           on the device whether or not usable_out is given).  Extraction needs no medians when |alpha| < pi/2 (the bit is then the
 *           side of the line through j and j+pi); with |alpha| >= pi/2 the batched extraction calls return
 *           TFFT_E_INVALID -- tfft_read_bins[_dev] with the image's medians covers that case.
 * (ctx, NULL, 0, 0) clears both.  Synchronises with the context's streams.  The single-image calls keep their own arguments. */
int tfft_set_phase_options(tfft_ctx* ctx, const float* jitter, uint64_t n, int adaptive_alpha);

/* Exact capacities of the BATCHED embeds.  By default their usable_out is the count on the fp32 planes of the
 * batch statistics, which can be 1-2 off the reference's integer (a bin within fp32 rounding of the threshold): near the boundary a caller
 * could accept or refuse a payload ("Message too large", S:1009-1012) differently from the reference.  This opt-in mode makes usable_out
 * the reference's integer, i.e. tfft_capacity(magmin * tfft_medians) of each image alone:
 *   TFFT_BATCH_EXACT_OFF  : default; the fp32 counts, same kernels and launch sequence as without the setter;
 *   TFFT_BATCH_EXACT_ALL  : every image of every call that fills usable_out is settled;
 *   TFFT_BATCH_EXACT_NEAR : only images whose fp32 count lies within guard_bits of the call's stream length (n_bits of the bit-level
 *                           calls, 912 + 56*payload_len of the stream calls): those whose decision the integer can change.  The default
 *                           guard, 64 bits, is far above the largest |fp32 - exact| the tests saw (1, 32 x 1080p and 8 x 4K).
 * Applies to tfft_embed_batch[_dev], tfft_embed_stream_batch[_dev], tfft_embed_stream_batch_walks[_dev], tfft_embed_stream_batch_fit[_dev]
 * (the cover's capacity) and so to tfp_embed_png_batch through the context.  The stego bytes do not change: the embed, adaptive alpha
 * included, keeps the fp32 batch medians.  With the mode on, a call that fills usable_out settles each chunk after its embed (a storing
 * forward of the selected covers, then the fp64 rounds of tfft_medians / tfft_capacity for all of them at once); it synchronises and is
 * never captured into or replayed from the graph cache (TFFT_GRAPHS).  Device buffers are allocated when the mode is first turned on.
 * A mode outside 0..2 gives TFFT_E_INVALID. */
#define TFFT_BATCH_EXACT_OFF  0   /* default: today's fp32 counts, bit for bit */
#define TFFT_BATCH_EXACT_ALL  1   /* every image's usable_out is the reference's integer */
#define TFFT_BATCH_EXACT_NEAR 2   /* only images whose fp32 count lies within guard_bits of the call's stream length */
int tfft_set_batch_exact(tfft_ctx* ctx, int mode, uint64_t guard_bits);
/* per image of the LAST batched embed call that filled usable_out: 1 exact, 0 fp32 count (mode off, not near, or no usable_out),
 * -1 exact was asked for but could not be settled (returns the fp32 count: candidate overflow, flat spectrum, PW > 8192, W < 2).
 * n_images larger than that call's gives TFFT_E_INVALID.  (tfp_embed_png_batch calls the context once per chunk: its last chunk's.) */
int tfft_batch_exact_info(const tfft_ctx* ctx, int n_images, int32_t* state_out);

/* ------------------------------------------------------------ measurement
 * Device-side timing of whatever was enqueued between the two calls on the
 * context's stream (hipEvent pair on that stream). */
int tfft_timer_begin(tfft_ctx* ctx);
int tfft_timer_end(tfft_ctx* ctx, float* ms);
/* Per-kernel timing for the roofline report: enqueue stage `stage` of the
 * batched pipeline over slots [0, n_images) `reps` times on the context's stream
 * between two HIP events; returns the mean time of ONE repetition (ms) and how
 * many kernel launches one repetition is.  Slot 0 must have been through a
 * forward call (its geometry is reused for the whole batch; results of the
 * repeated stage are discarded by the caller).  Stages: 0 rows_fwd, 1 cols_fwd
 * step A (or the direct column pass), 2 cols_fwd step B, 3 embed, 4 cols_inv
 * step A, 5 cols_inv step B, 6 rows_inv, 7 read, 8 medians (with the capacity
 * count of the batch path inside its full pass), 9 capacity as a pass of its own
 * (0 launches in the default configuration), 10 the final forward column step as
 * extraction runs it. */
int tfft_profile_stage(tfft_ctx* ctx, int n_images, int stage, int reps, const void* rgb_dev, void* rgb_out_dev,
                       const void* bins_dev, const void* bits_dev, void* bits_out_dev, uint64_t n_bits, double alpha,
                       float* ms_per_rep, int* n_launches);

#ifdef __cplusplus
}
#endif
#endif /* TURTLEFFT_HIP_H */
