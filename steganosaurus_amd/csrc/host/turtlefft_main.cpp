// turtlefft_main.cpp -- the `turtlefft embed | extract | gen-key` command line of
// rickenator/steganosaurus, re-implemented as a host driver around the MI355X library
// (include/turtlefft_hip.h).  Command grammar, defaults (struct Params, S:375-381),
// success/error messages and exit codes follow steganosaur.cpp:813-877, 907-1426 so that
// scripts written for the reference keep working; the signal path (planes, FFT, medians,
// capacity, phase embed/read, inverse) runs on the GPU through the C ABI, the keyed walk,
// framing, ECC and crypto run on the host.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../../include/turtlefft_hip.h"
#include "tf_crypto.h"
#include "tf_frame.h"
#include "tf_png.h"

using namespace tfh;

namespace {

struct Params {     // S:375-381
    double alpha = 0.50, rmin = 0.05, rmax = 0.45, magmin = 0.01, density = 0.7, jitter = 0.0;
    bool center = false;
    uint32_t pbkdf2_iter = 600000;
    bool adaptive_alpha = false;
    bool cover_dependent_path = false;
    bool fit_crop = false;          // embed only, not in the reference: fit the stego so that it survives the crop to W x H
    bool report = false;            // embed only, not in the reference: PSNR / SSIM / phase-histogram KL of the written stego on stderr
};
struct Args {       // S:839-845
    std::string mode, inPath, outPath, secret, pass, keyBase64, keyOutPath, wrapPass;
    std::string robust;             // embed only, not in the reference: --robust SPEC, the channels the written stego is tested against
    std::vector<tfft_channel> channels;      // ... parsed, and each channel's own text
    std::vector<std::string> channel_names;
    Params P;
};

void usage() {
    fprintf(stderr,
            "Usage:\n"
            "  turtlefft gen-key [--key-out FILE] [--wrap-pass PW]\n"
            "      Generate a 256-bit master key; print base64 and fingerprint; optionally export it\n"
            "      (wrapped with ChaCha20-Poly1305 under PW when --wrap-pass is given).\n"
            "  turtlefft embed   --in host.png --out stego.png --secret TEXT (--pass PW | --key KEY_BASE64)\n"
            "      [--alpha 0.5 --jitter 0 --density 0.7 --rmin 0.05 --rmax 0.45 --magmin 0.01 --center 0]\n"
            "      [--pbkdf2_iter 600000 --adaptive_alpha 0 --cover_dependent_path 0 --wrap-pass PW]\n"
            "      [--fit_crop 0]  1: fit the stego so that covers whose sides are not powers of two read back\n"
            "      [--report 0]    1: print PSNR, SSIM and the annulus phase-histogram KL(stego||cover) per plane on stderr\n"
            "      [--robust SPEC] read the written stego back through channels and print the error counts on stderr;\n"
            "                      SPEC = comma list of none | awgn:SIGMA[:SEED] | jpeg:Q   (e.g. none,awgn:2:7,jpeg:75)\n"
            "  turtlefft extract --in stego.png (--pass PW | --key KEY_BASE64)\n"
            "      [same tuning options as embed]\n"
            "  turtlefft spam    --in image.png\n"
            "      Print the 686 second-order SPAM features (T = 3) of each plane, one line R, G, B: what a blind\n"
            "      spatial-domain steganalyser's classifier eats.\n"
            "  The 2-D FFT / phase embedding runs on an AMD MI355X through libturtlefft_hip.so.\n");
}

// ---- command line: one table row per option (the grammar, defaults and failure modes are the reference's, S:813-877: every
// option takes exactly one value, unknown options print `Unknown arg: X` + usage, flags are "1" / "true")
enum class OptKind { Text, Real, Flag, Count };
struct OptSpec {
    const char* name;
    OptKind kind;
    std::string Args::*text;          // Text
    double Params::*real;             // Real
    bool Params::*flag;               // Flag
    uint32_t Params::*count;          // Count
};
const OptSpec kOptions[] = {
    {"--in", OptKind::Text, &Args::inPath, nullptr, nullptr, nullptr},
    {"--out", OptKind::Text, &Args::outPath, nullptr, nullptr, nullptr},
    {"--secret", OptKind::Text, &Args::secret, nullptr, nullptr, nullptr},
    {"--pass", OptKind::Text, &Args::pass, nullptr, nullptr, nullptr},
    {"--key", OptKind::Text, &Args::keyBase64, nullptr, nullptr, nullptr},
    {"--key-out", OptKind::Text, &Args::keyOutPath, nullptr, nullptr, nullptr},
    {"--wrap-pass", OptKind::Text, &Args::wrapPass, nullptr, nullptr, nullptr},
    {"--robust", OptKind::Text, &Args::robust, nullptr, nullptr, nullptr},
    {"--alpha", OptKind::Real, nullptr, &Params::alpha, nullptr, nullptr},
    {"--jitter", OptKind::Real, nullptr, &Params::jitter, nullptr, nullptr},
    {"--density", OptKind::Real, nullptr, &Params::density, nullptr, nullptr},
    {"--rmin", OptKind::Real, nullptr, &Params::rmin, nullptr, nullptr},
    {"--rmax", OptKind::Real, nullptr, &Params::rmax, nullptr, nullptr},
    {"--magmin", OptKind::Real, nullptr, &Params::magmin, nullptr, nullptr},
    {"--center", OptKind::Flag, nullptr, nullptr, &Params::center, nullptr},
    {"--adaptive_alpha", OptKind::Flag, nullptr, nullptr, &Params::adaptive_alpha, nullptr},
    {"--cover_dependent_path", OptKind::Flag, nullptr, nullptr, &Params::cover_dependent_path, nullptr},
    {"--fit_crop", OptKind::Flag, nullptr, nullptr, &Params::fit_crop, nullptr},
    {"--report", OptKind::Flag, nullptr, nullptr, &Params::report, nullptr},
    {"--pbkdf2_iter", OptKind::Count, nullptr, nullptr, nullptr, &Params::pbkdf2_iter},
};

const OptSpec* find_option(const char* name) {
    for (const OptSpec& o : kOptions)
        if (strcmp(o.name, name) == 0) return &o;
    return nullptr;
}

// --robust SPEC: a comma list of none | awgn:SIGMA[:SEED] | jpeg:Q.  Anything else (an empty item, an unknown channel, a number with a tail,
// sigma < 0, Q outside 1..100) is a usage error
bool parse_number(const std::string& t, double& v) {
    if (t.empty()) return false;
    char* end = nullptr;
    v = strtod(t.c_str(), &end);
    return end && *end == '\0' && std::isfinite(v);
}
bool parse_channels(const std::string& spec, std::vector<tfft_channel>& out, std::vector<std::string>& names) {
    size_t pos = 0;
    while (pos <= spec.size()) {
        const size_t comma = std::min(spec.find(',', pos), spec.size());
        const std::string item = spec.substr(pos, comma - pos);
        pos = comma + 1;
        std::vector<std::string> f;
        for (size_t a = 0; a <= item.size();) { const size_t c = std::min(item.find(':', a), item.size()); f.push_back(item.substr(a, c - a)); a = c + 1; }
        tfft_channel ch{0, 0.0f, 0};
        double v = 0.0;
        if (f[0] == "none" && f.size() == 1) ch.kind = 0;
        else if (f[0] == "awgn" && (f.size() == 2 || f.size() == 3)) {
            if (!parse_number(f[1], v) || v < 0.0) return false;
            ch.kind = 1; ch.param = (float)v;
            if (f.size() == 3) {
                if (f[2].empty() || f[2].find_first_not_of("0123456789") != std::string::npos || f[2].size() > 19) return false;
                ch.seed = strtoull(f[2].c_str(), nullptr, 10);
            }
        } else if (f[0] == "jpeg" && f.size() == 2) {
            if (!parse_number(f[1], v) || v < 1.0 || v > 100.0 || v != floor(v)) return false;
            ch.kind = 2; ch.param = (float)v;
        } else return false;
        out.push_back(ch);
        names.push_back(item);
    }
    return !out.empty();
}

bool parse_args(int argc, char** argv, Args& A) {
    if (argc < 2) return false;
    A.mode = argv[1];
    int i = 2;
    while (i < argc) {
        const OptSpec* o = find_option(argv[i]);
        if (!o) { fprintf(stderr, "Unknown arg: %s\n", argv[i]); return false; }
        const std::string value = (i + 1 < argc) ? argv[i + 1] : "";      // a trailing option without a value reads as empty
        i += 2;
        switch (o->kind) {
            case OptKind::Text: A.*(o->text) = value; break;
            case OptKind::Real: A.P.*(o->real) = std::stod(value); break;               // throws on garbage: main() prints usage
            case OptKind::Flag: A.P.*(o->flag) = (value == "1" || value == "true"); break;
            case OptKind::Count: A.P.*(o->count) = (uint32_t)std::stoul(value); break;
        }
    }
    if (!A.robust.empty() && !parse_channels(A.robust, A.channels, A.channel_names)) return false;
    // what each mode cannot do without
    const bool has_secret_source = !A.pass.empty() || !A.keyBase64.empty();
    if (A.mode == "gen-key") return true;
    if (A.mode == "extract") return !A.inPath.empty() && has_secret_source;
    if (A.mode == "spam") return !A.inPath.empty();
    if (A.mode == "embed") return !A.inPath.empty() && has_secret_source && !A.outPath.empty() && !A.secret.empty();
    return false;
}

[[noreturn]] void die(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
void die(const char* fmt, ...) {
    va_list ap; va_start(ap, fmt); vfprintf(stderr, fmt, ap); va_end(ap);
    fputc('\n', stderr);
    exit(1);
}
void tf(int rc, const char* what) {
    if (rc != TFFT_OK) die("%s: %s", what, tfft_strerror(rc));
}

// 80-byte wrapped key: "TFKW" salt16 nonce12 ct32 tag16, or a raw 32-byte key, base64 (S:594-662)
bool decode_or_unwrap_key(const std::string& key_data, const std::string& unwrap_pass, uint32_t iters,
                          std::array<uint8_t, 32>& key_out) {
    std::vector<uint8_t> d;
    if (!base64_decode(key_data, d)) return false;
    if (d.empty() && !key_data.empty()) return false;
    if (d.size() == 80 && memcmp(d.data(), "TFKW", 4) == 0) {
        if (unwrap_pass.empty()) { fprintf(stderr, "Key is wrapped but no unwrap passphrase provided\n"); return false; }
        uint8_t derived[44];
        pbkdf2_hmac_sha256((const uint8_t*)unwrap_pass.data(), unwrap_pass.size(), d.data() + 4, 16, iters, derived, 44);
        const bool ok = aead_open_turtle(derived, d.data() + 20, nullptr, 0, d.data() + 32, 32, d.data() + 64, key_out.data());
        secure_zero(derived, sizeof derived);
        return ok;
    }
    if (d.size() == 32) { memcpy(key_out.data(), d.data(), 32); return true; }
    return false;
}

struct Spectrum {        // a resident image on the device + everything derived from the key
    tfft_ctx* ctx = nullptr;
    int W = 0, H = 0, PW = 0, PH = 0;
    double med[3] = {0, 0, 0};
    std::array<uint8_t, 32> path_key;
    uint8_t sub[128];
    ~Spectrum() { if (ctx) tfft_destroy(ctx); secure_zero(sub, sizeof sub); }
};

// S:909-923 / S:1114-1131 and S:1020-1066: load, forward transform, medians, path key, sub-keys
void open_image(const Args& A, Spectrum& S, const std::vector<uint8_t>& rgb, bool using_raw_key,
                const std::array<uint8_t, 32>& master_key) {
    int dev = 0;
    if (const char* e = getenv("TURTLEFFT_DEVICE")) dev = atoi(e);
    tf(tfft_create(dev, S.W, S.H, 1, &S.ctx), "turtlefft: cannot open the GPU context");
    tf(tfft_forward_rgb8(S.ctx, 0, rgb.data(), S.W, S.H, A.P.center, &S.PW, &S.PH), "forward transform");
    tf(tfft_medians(S.ctx, 0, S.med), "medians");
    const uint8_t* sec = using_raw_key ? master_key.data() : (const uint8_t*)A.pass.data();
    const size_t sec_n = using_raw_key ? 32 : A.pass.size();
    if (A.P.cover_dependent_path) {      // S:415-444 on the resident spectrum: 8x8 low-frequency magnitudes
        const int region = std::min(8, std::min(S.PH, S.PW) / 8);
        std::vector<double> mags((size_t)3 * region * region);
        if (region > 0) tf(tfft_lowfreq_mag(S.ctx, 0, region, mags.data()), "cover hash");
        const auto ch = cover_hash_from_mags(mags.data(), mags.size());
        S.path_key = path_key_of(sec, sec_n, ch.data());
    } else {
        S.path_key = path_key_of(sec, sec_n, nullptr);
    }
    turtle_subkeys(S.path_key, S.sub);
}

// --report 1: one line on stderr comparing the cover with the bytes just written -- PSNR and SSIM per plane (tfft_quality_batch) and
// KL(stego || cover) of the 256-bin annulus phase histograms (tfft_phase_hist_batch, no magnitude test), smoothed as
// steganosaurus_amd.analysis.kl_divergence: P = (c + 0.5) / (N + 0.5 nb), natural log
void report_line(const Args& A, Spectrum& S, const std::vector<uint8_t>& cover, const std::vector<uint8_t>& stego) {
    constexpr int NB = 256;
    const bool ssim_ok = S.W >= 11 && S.H >= 11;
    uint64_t sse[3];
    double ssim[3];
    tf(tfft_quality_batch(S.ctx, 1, cover.data(), stego.data(), S.W, S.H, sse, ssim_ok ? ssim : nullptr), "report");
    std::vector<uint32_t> hc(3 * NB), hs(3 * NB);
    tf(tfft_phase_hist_batch(S.ctx, 1, cover.data(), S.W, S.H, A.P.center, A.P.rmin, A.P.rmax, nullptr, NB, hc.data()), "report");
    tf(tfft_phase_hist_batch(S.ctx, 1, stego.data(), S.W, S.H, A.P.center, A.P.rmin, A.P.rmax, nullptr, NB, hs.data()), "report");
    std::string line = "Report: PSNR(dB)";
    char buf[64];
    const char* names[3] = {"R", "G", "B"};
    for (int p = 0; p < 3; p++) {
        if (sse[p] == 0) snprintf(buf, sizeof buf, " %s=inf", names[p]);
        else snprintf(buf, sizeof buf, " %s=%.6f", names[p], 10.0 * log10(255.0 * 255.0 * (double)S.W * (double)S.H / (double)sse[p]));
        line += buf;
    }
    line += "; SSIM";
    for (int p = 0; p < 3; p++) {
        if (ssim_ok) snprintf(buf, sizeof buf, " %s=%.6f", names[p], ssim[p]);
        else snprintf(buf, sizeof buf, " %s=n/a", names[p]);
        line += buf;
    }
    line += "; KL(stego||cover)";
    for (int p = 0; p < 3; p++) {
        double np_ = 0.0, nq = 0.0, kl = 0.0;
        for (int i = 0; i < NB; i++) { np_ += hs[p * NB + i]; nq += hc[p * NB + i]; }
        for (int i = 0; i < NB; i++) {
            const double P = (hs[p * NB + i] + 0.5) / (np_ + 0.5 * NB), Q = (hc[p * NB + i] + 0.5) / (nq + 0.5 * NB);
            kl += P * log(P / Q);
        }
        snprintf(buf, sizeof buf, " %s=%.8f", names[p], kl);
        line += buf;
    }
    fprintf(stderr, "%s\n", line.c_str());
}

// the header and payload bytes of a framed stream, out of its repetition code: every 3rd / 7th bit
void unframe(const std::vector<uint8_t>& bits, std::vector<uint8_t>& header, std::vector<uint8_t>& payload) {
    std::vector<uint8_t> hb(HEADER_LEN * 8), pb((bits.size() - HEADER_LEN * 24) / 7);
    for (size_t i = 0; i < hb.size(); i++) hb[i] = bits[3 * i];
    for (size_t i = 0; i < pb.size(); i++) pb[i] = bits[HEADER_LEN * 24 + 7 * i];
    header = bytes_from_bits(hb);
    payload = bytes_from_bits(pb);
}

// --robust SPEC: one line on stderr -- the bytes just written through every channel of the spec, read back along the walk just used
// (tfft_robustness_batch; jitter and adaptive alpha through the phase options): raw bit errors of the stream, header and payload byte errors
// after the repetition code, and whether the message came back.  Never changes the exit code: a refusal is reported on the same line
void robust_line(const Args& A, Spectrum& S, const std::vector<uint8_t>& stego, const std::vector<tfft_bin>& bins, const std::vector<float>& jit,
                 const std::vector<uint8_t>& bits) {
    std::vector<uint8_t> header, payload;
    unframe(bits, header, payload);
    const size_t n = A.channels.size();
    std::vector<uint32_t> res(n * 4);
    int rc = tfft_set_phase_options(S.ctx, jit.empty() ? nullptr : jit.data(), bins.size(), A.P.adaptive_alpha);
    if (rc == TFFT_OK)
        rc = tfft_robustness_batch(S.ctx, 1, stego.data(), S.W, S.H, A.P.center, bins.data(), bins.size(), A.P.alpha, header.data(), payload.data(),
                                   payload.size(), A.channels.data(), (int)n, 0, res.data());
    if (rc != TFFT_OK) { fprintf(stderr, "Robustness: not measured (%s)\n", tfft_strerror(rc)); return; }
    std::string line = "Robustness:";
    char buf[160];
    for (size_t k = 0; k < n; k++) {
        const uint32_t* r = &res[4 * k];
        const bool ok = r[1] == 0 && r[2] == 0 && (int32_t)r[3] == (int32_t)payload.size() - 16;
        snprintf(buf, sizeof buf, "%s %s raw=%u/%zu hdr=%u/%u pay=%u/%zu %s", k ? ";" : "", A.channel_names[k].c_str(), r[0], bits.size(), r[1],
                 (unsigned)HEADER_LEN, r[2], payload.size(), ok ? "ok" : "lost");
        line += buf;
    }
    fprintf(stderr, "%s\n", line.c_str());
}

void do_embed(const Args& A) {      // S:907-1109
    const bool using_raw_key = !A.keyBase64.empty();
    std::array<uint8_t, 32> master_key{};
    Spectrum S;
    std::vector<uint8_t> rgb;      // the reference loads the image before it looks at the key (S:909 vs S:935)
    if (!load_rgb8(A.inPath, rgb, S.W, S.H)) die("Failed to load %s", A.inPath.c_str());
    if (using_raw_key && !decode_or_unwrap_key(A.keyBase64, A.wrapPass, A.P.pbkdf2_iter, master_key))
        die("Failed to decode/unwrap key from --key argument");
    open_image(A, S, rgb, using_raw_key, master_key);
    if (!A.P.fit_crop && !A.P.report) std::vector<uint8_t>().swap(rgb);      // (the fitted embed adds to the cover again and again; the report compares)

    std::array<uint8_t, 16> salt{};
    { std::random_device rd; for (auto& b : salt) b = (uint8_t)rd(); }                  // S:927-929
    const KeyMaterial km = using_raw_key ? derive_keys_from_raw(master_key, salt) : derive_keys(A.pass, salt, A.P.pbkdf2_iter);
    secure_zero(master_key.data(), master_key.size());
    const std::vector<uint8_t> bits = frame_stream(km, A.secret);

    const double thr[3] = {A.P.magmin * S.med[0], A.P.magmin * S.med[1], A.P.magmin * S.med[2]};   // S:923
    uint64_t usable = 0;
    tf(tfft_capacity(S.ctx, 0, A.P.rmin, A.P.rmax, thr, &usable), "capacity");
    if (bits.size() > usable)
        die("Message too large. Need %zu bits (after ECC), capacity ~%zu bits.", bits.size(), (size_t)usable);

    tfft_walk* wk = nullptr;
    tf(tfft_walk_create(S.sub, S.PH, S.PW, A.P.rmin, A.P.rmax, A.P.density, &wk), "walk");
    std::vector<tfft_bin> bins(bits.size());
    tf(tfft_walk_next(wk, bins.size(), bins.data(), nullptr), "walk");
    tfft_walk_destroy(wk);
    std::vector<float> jit;
    if (A.P.jitter != 0.0) {
        jit.resize(bins.size());
        tf(tfft_walk_jitter(S.sub + 32, bins.data(), bins.size(), A.P.jitter, jit.data()), "jitter");
    }
    std::vector<uint8_t> out((size_t)S.W * S.H * 3);
    if (A.P.fit_crop) {
        // the walk and jitter above through the fitted batch embed (one image), with the stream's header and payload bytes
        std::vector<uint8_t> header, payload;
        unframe(bits, header, payload);
        int32_t iters = 0;
        uint32_t wrong = 0;
        tf(tfft_embed_stream_batch_fit(S.ctx, 1, rgb.data(), S.W, S.H, A.P.center, bins.data(), jit.empty() ? nullptr : jit.data(), bins.size(),
                                       A.P.adaptive_alpha, header.data(), payload.data(), payload.size(), A.P.alpha, A.P.rmin, A.P.rmax,
                                       A.P.magmin, 16, 0.5, nullptr, &iters, &wrong, out.data()), "embed");
        if (iters < 0) fprintf(stderr, "Warning: the fitted stego did not converge; %u of %zu stream bits read wrong.\n", wrong, bits.size());
    } else {
        tf(tfft_embed_bins(S.ctx, 0, bins.data(), bits.data(), jit.empty() ? nullptr : jit.data(), bins.size(), A.P.alpha,
                           A.P.adaptive_alpha, S.med), "embed");
        tf(tfft_inverse_rgb8(S.ctx, 0, out.data()), "inverse transform");
    }
    if (!png_write_rgb8(A.outPath, out.data(), S.W, S.H)) die("PNG write failed: %s", A.outPath.c_str());
    fprintf(stdout, "Embedded %zu bits into %s (payload %u bytes, ver=2, salt/nonce in header)\n", bits.size(),
            A.outPath.c_str(), (unsigned)A.secret.size());
    if (A.P.report) report_line(A, S, rgb, out);
    if (!A.channels.empty()) robust_line(A, S, out, bins, jit, bits);
}

void do_extract(const Args& A) {    // S:1112-1312
    const bool using_raw_key = !A.keyBase64.empty();
    std::array<uint8_t, 32> master_key{};
    Spectrum S;
    std::vector<uint8_t> rgb;
    if (!load_rgb8(A.inPath, rgb, S.W, S.H)) die("Failed to load %s", A.inPath.c_str());
    if (using_raw_key && !decode_or_unwrap_key(A.keyBase64, A.wrapPass, A.P.pbkdf2_iter, master_key))
        die("Failed to decode/unwrap key from --key argument");
    open_image(A, S, rgb, using_raw_key, master_key);
    std::vector<uint8_t>().swap(rgb);

    tfft_walk* wk = nullptr;
    tf(tfft_walk_create(S.sub, S.PH, S.PW, A.P.rmin, A.P.rmax, A.P.density, &wk), "walk");
    uint64_t walked = 0;
    auto read_bits = [&](size_t n) {      // the read_next_bit loop, n positions further along the SAME walk (S:1205-1226)
        std::vector<tfft_bin> bins(n);
        const int rc = tfft_walk_next(wk, n, bins.data(), nullptr);
        if (rc == TFFT_E_EXHAUSTED) die("Payload truncated after ECC decode.");   // the reference would spin forever here
        tf(rc, "walk");
        std::vector<float> jit;
        if (A.P.jitter != 0.0) {
            // the per-plane jitter streams continue across calls: regenerate from the start and keep the tail
            std::vector<tfft_bin> all;   // (only paid when --jitter is used)
            tfft_walk* w2 = nullptr;
            tf(tfft_walk_create(S.sub, S.PH, S.PW, A.P.rmin, A.P.rmax, A.P.density, &w2), "walk");
            all.resize(walked + n);
            tf(tfft_walk_next(w2, all.size(), all.data(), nullptr), "walk");
            tfft_walk_destroy(w2);
            std::vector<float> ja(all.size());
            tf(tfft_walk_jitter(S.sub + 32, all.data(), all.size(), A.P.jitter, ja.data()), "jitter");
            jit.assign(ja.begin() + (ptrdiff_t)walked, ja.end());
        }
        walked += n;
        std::vector<uint8_t> bits(n);
        tf(tfft_read_bins(S.ctx, 0, bins.data(), jit.empty() ? nullptr : jit.data(), n, A.P.alpha, A.P.adaptive_alpha, S.med,
                          bits.data()), "read");
        return bits;
    };

    bool ok = true;
    const std::vector<uint8_t> hdr_bits = rep_decode(read_bits(HEADER_LEN * 8 * 3), 3, ok);
    if (!ok) die("Header ECC length mismatch.");
    const std::vector<uint8_t> hdr = bytes_from_bits(hdr_bits);
    if (hdr.size() < HEADER_LEN) die("Header truncated.");
    if (!(hdr[0] == 'F' && hdr[1] == 'T' && hdr[2] == 'T' && hdr[3] == 'G')) die("Magic not found.");
    if (hdr[4] != 2) die("Unsupported version (%u).", hdr[4]);
    const uint32_t clen = ((uint32_t)hdr[34] << 24) | ((uint32_t)hdr[35] << 16) | ((uint32_t)hdr[36] << 8) | hdr[37];
    const size_t rest_bytes = (size_t)clen + 16;
    // a corrupt header can claim up to 4 GiB: bound the request by what the annulus can hold at all
    // (the reference allocates and walks blindly)
    if (rest_bytes * 56 > (size_t)3 * S.PH * S.PW) die("Payload truncated after ECC decode.");
    const std::vector<uint8_t> pay_bits = rep_decode(read_bits(rest_bytes * 8 * 7), 7, ok);
    if (!ok) die("Payload rep7 decode failed.");
    const std::vector<uint8_t> rest = bytes_from_bits(pay_bits);
    if (rest.size() < rest_bytes) die("Payload truncated after ECC decode.");
    tfft_walk_destroy(wk);

    std::array<uint8_t, 16> salt; memcpy(salt.data(), &hdr[6], 16);
    const KeyMaterial km = using_raw_key ? derive_keys_from_raw(master_key, salt) : derive_keys(A.pass, salt, A.P.pbkdf2_iter);
    secure_zero(master_key.data(), master_key.size());
    std::string secret(clen, '\0');
    // authenticated with the RECEIVED header bytes as AAD and the DERIVED nonce (S:1299-1307)
    if (!aead_open_turtle(km.aead_key.data(), km.nonce.data(), hdr.data(), HEADER_LEN, rest.data(), clen, rest.data() + clen,
                   (uint8_t*)&secret[0]))
        die("Auth failed (wrong pass or data corrupted).");
    printf("%s\n", secret.c_str());
}

// `spam --in IMAGE`, not in the reference: the SPAM features of steganosaurus_amd.analysis.spam_features at T = 3, from
// the counts of tfft_spam_batch -- per direction M = C / sum(C) (0 for an empty direction), the opposite direction by the index
// permutation [a, b, c] <- [-c, -b, -a], the mean over right, left, down, up and then over the four diagonals
void do_spam(const Args& A) {
    constexpr int T = 3, N = 2 * T + 1, N3 = N * N * N;
    int W = 0, H = 0;
    std::vector<uint8_t> rgb;
    if (!load_rgb8(A.inPath, rgb, W, H)) die("Failed to load %s", A.inPath.c_str());
    int dev = 0;
    if (const char* e = getenv("TURTLEFFT_DEVICE")) dev = atoi(e);
    tfft_ctx* ctx = nullptr;
    tf(tfft_create(dev, W, H, 1, &ctx), "turtlefft: cannot open the GPU context");
    std::vector<uint32_t> counts((size_t)3 * 4 * N3);
    tf(tfft_spam_batch(ctx, 1, rgb.data(), W, H, T, counts.data()), "spam");
    tfft_destroy(ctx);
    const char* names[3] = {"R", "G", "B"};
    for (int p = 0; p < 3; p++) {
        std::vector<double> both((size_t)4 * N3, 0.0);      // M_d + M_{-d}
        for (int d = 0; d < 4; d++) {
            const uint32_t* c = &counts[(size_t)(p * 4 + d) * N3];
            double tot = 0.0;
            for (int i = 0; i < N3; i++) tot += (double)c[i];
            if (tot <= 0.0) continue;
            for (int a = 0; a < N; a++)
                for (int b = 0; b < N; b++)
                    for (int e = 0; e < N; e++) {
                        const int i = (a * N + b) * N + e, o = ((N - 1 - e) * N + (N - 1 - b)) * N + (N - 1 - a);
                        both[(size_t)d * N3 + i] = (double)c[i] / tot + (double)c[o] / tot;
                    }
        }
        fputs(names[p], stdout);
        for (int half = 0; half < 2; half++)
            for (int i = 0; i < N3; i++)
                printf(" %.9e", (both[(size_t)(2 * half) * N3 + i] + both[(size_t)(2 * half + 1) * N3 + i]) / 4.0);
        fputc('\n', stdout);
    }
}

void do_gen_key(const Args& A) {    // S:1315-1416
    std::array<uint8_t, 32> master{};
    if (!random_bytes(master.data(), 32)) die("Failed to generate random key (CSPRNG error)");
    const auto fp = sha256(master.data(), 32);
    const std::string b64 = base64_encode(master.data(), 32);
    printf("Generated 256-bit master key:\n  Base64: %s\n  Fingerprint: %s\n", b64.c_str(), to_hex(fp.data(), 8).c_str());
    if (!A.keyOutPath.empty()) {
        std::string text;
        if (!A.wrapPass.empty()) {
            uint8_t salt[16], derived[44];
            if (!random_bytes(salt, 16)) die("Failed to generate salt");
            pbkdf2_hmac_sha256((const uint8_t*)A.wrapPass.data(), A.wrapPass.size(), salt, 16, A.P.pbkdf2_iter, derived, 44);
            std::vector<uint8_t> blob = {'T', 'F', 'K', 'W'};
            blob.insert(blob.end(), salt, salt + 16);
            blob.insert(blob.end(), derived + 32, derived + 44);
            blob.resize(80);
            aead_seal_turtle(derived, derived + 32, nullptr, 0, master.data(), 32, &blob[32], &blob[64]);
            secure_zero(derived, sizeof derived);
            text = base64_encode(blob.data(), blob.size()) + "\n";
            printf("  Wrapped with passphrase and exported to: %s\n", A.keyOutPath.c_str());
        } else {
            text = b64 + "\n";
            printf("  Exported (unencrypted) to: %s\n", A.keyOutPath.c_str());
        }
        FILE* f = fopen(A.keyOutPath.c_str(), "wb");
        if (!f) die("Failed to open %s for writing", A.keyOutPath.c_str());
        const bool ok = fwrite(text.data(), 1, text.size(), f) == text.size();
        fclose(f);
        if (!ok) die("Failed to write key file");
    }
    secure_zero(master.data(), 32);
}

}  // namespace

int main(int argc, char** argv) {
    Args A;
    try {
        if (!parse_args(argc, argv, A)) { usage(); return 1; }
    } catch (const std::exception&) {      // the reference lets std::stod throw on a missing/garbled value (uncaught -> abort)
        usage();
        return 1;
    }
    if (A.mode == "gen-key") do_gen_key(A);
    else if (A.mode == "embed") do_embed(A);
    else if (A.mode == "spam") do_spam(A);
    else do_extract(A);
    return 0;
}
