// Host-side synthetic job-batch encoder for the end-to-end ingest window.
//
// Plain C++17, no torch / HIP dependency: the extension wrapper
// (cordum_kernels.hip) and the stand-alone sanitizer programs
// (tests/native/encode_check.cpp, encode_compact_check.cpp) include this file.
//
// Draws are those of synthetic_fresh, bit for bit: per job i,
//   h0 = splitmix64(base ^ i), h1 = splitmix64(h0), h2 = splitmix64(h1)
//   base = splitmix64(seed * 0x5851F42D4C957F2D ^ step)
// tenant/topic/risk/requires indices are Lemire multiply-shift reductions of
// the four 32-bit halves of h0/h1, the risk / requires coin flips compare the
// halves of h2 against fixed cut-offs. Only the four synthetic dims of a row
// are written; the other dims are left as they are.
//
// One loop serves two destination layouts. Full: `any` is [B,7,W], `all` is
// [B,2,W] and dim_* / all_requires index the dim inside a row (the default:
// strides 0). Compact: both base pointers are the same [B,L] array of the
// columns the compiled policy reads, both strides are L, and dim_* /
// all_requires are column numbers; a negative one means the policy does not
// read that dim, and its store is skipped (the draws are made all the same,
// so every other value is what the full layout gets).
//
// What is different from the serial loop is the schedule, not the values:
// jobs are hashed a block at a time into small arrays (a loop the compiler
// vectorizes: three splitmix rounds and four multiply-shifts over 64 lanes),
// then a second loop does the LUT gathers and the row stores. The block loop
// also stamps word 0 of each payload row with the step, so one GIL-free call
// prepares the whole batch. A batch can be split over two threads owned by
// the call (no shared pool: concurrent encodes must not serialize).
//
// The object code is built on one machine and run on another, so nothing
// here assumes the build host's ISA: the block loop is compiled three times
// (baseline, AVX2, AVX-512DQ) and picked by a runtime CPU check.
#pragma once

#include <cstddef>
#include <cstdint>
#include <thread>

namespace cordum_enc {

struct EncodeJob {
    int64_t* any;            // [B,7,W], or rows of any_stride*W words
    int64_t* all;            // [B,2,W], or rows of all_stride*W words
    const int64_t* tenant_lut;  // [V,W]
    const int64_t* topic_lut;
    const int64_t* risk_lut;
    const int64_t* req_lut;
    int64_t B, W, V;
    uint64_t seed, step;
    // destination offset of each synthetic dim inside its row, in units of W
    // words (tenant/topic/risk from `any`, requires from `all`); < 0: skip
    int dim_tenant, dim_topic, dim_risk, all_requires;
    int32_t* payload;        // [B,payload_words] or nullptr: no stamp
    int64_t payload_words;
    // row strides of `any` / `all` in units of W words; 0: the full layout's
    // 7 and 2, so a value-initialised EncodeJob writes [B,7,W] / [B,2,W]
    int64_t any_stride = 0;
    int64_t all_stride = 0;
};

constexpr int kBlock = 64;
constexpr uint32_t kRiskCut = 1288490189u;  // 0.30 * 2^32
constexpr uint32_t kReqCut = 429496730u;    // 0.10 * 2^32

static inline uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

static inline uint64_t batch_base(uint64_t seed, uint64_t step) {
    return splitmix64(seed * 0x5851F42D4C957F2Dull ^ step);
}

// jobs [i0, i1) of the batch; always_inline so each ISA wrapper below gets
// its own copy compiled with that wrapper's target features
__attribute__((always_inline)) static inline void encode_range_impl(
    const EncodeJob& a, int64_t i0, int64_t i1)
{
    const uint64_t base = batch_base(a.seed, a.step);
    const uint64_t v = (uint64_t)a.V;
    const int64_t W = a.W;
    const int64_t sa = a.any_stride > 0 ? a.any_stride : 7;
    const int64_t sl = a.all_stride > 0 ? a.all_stride : 2;
    const bool st = a.dim_tenant >= 0, so = a.dim_topic >= 0;
    const bool sr = a.dim_risk >= 0, sq = a.all_requires >= 0;
    const int32_t stamp = (int32_t)(uint32_t)a.step;
    uint32_t t_idx[kBlock], o_idx[kBlock], r_idx[kBlock], q_idx[kBlock];
    uint32_t c_risk[kBlock], c_req[kBlock];
    for (int64_t b0 = i0; b0 < i1; b0 += kBlock) {
        const int n = (int)((i1 - b0) < kBlock ? (i1 - b0) : kBlock);
        // phase 1: hash (vectorizable; full block even on a tail, the extra
        // lanes are never read)
        for (int k = 0; k < kBlock; ++k) {
            const uint64_t h0 = splitmix64(base ^ (uint64_t)(b0 + k));
            const uint64_t h1 = splitmix64(h0);
            const uint64_t h2 = splitmix64(h1);
            t_idx[k] = (uint32_t)(((h0 & 0xffffffffull) * v) >> 32);
            o_idx[k] = (uint32_t)(((h0 >> 32) * v) >> 32);
            r_idx[k] = (uint32_t)(((h1 & 0xffffffffull) * v) >> 32);
            q_idx[k] = (uint32_t)(((h1 >> 32) * v) >> 32);
            c_risk[k] = (uint32_t)h2;
            c_req[k] = (uint32_t)(h2 >> 32);
        }
        // phase 2: gathers + row stores (none where no dim has a
        // destination: the row pointers may then be null)
        if (!(st || so || sr || sq)) {
        } else if (W == 1) {
            int64_t* arow = a.any + (size_t)b0 * sa;
            int64_t* lrow = a.all + (size_t)b0 * sl;
            for (int k = 0; k < n; ++k, arow += sa, lrow += sl) {
                if (st) arow[a.dim_tenant] = a.tenant_lut[t_idx[k]];
                if (so) arow[a.dim_topic] = a.topic_lut[o_idx[k]];
                if (sr) arow[a.dim_risk] = c_risk[k] < kRiskCut ? a.risk_lut[r_idx[k]] : 0;
                if (sq) lrow[a.all_requires] = c_req[k] < kReqCut ? a.req_lut[q_idx[k]] : 0;
            }
        } else {
            for (int k = 0; k < n; ++k) {
                int64_t* arow = a.any + (size_t)(b0 + k) * sa * W;
                int64_t* lrow = a.all + (size_t)(b0 + k) * sl * W;
                const bool has_risk = c_risk[k] < kRiskCut;
                const bool has_req = c_req[k] < kReqCut;
                const int64_t* tl = a.tenant_lut + (size_t)t_idx[k] * W;
                const int64_t* ol = a.topic_lut + (size_t)o_idx[k] * W;
                const int64_t* rl = a.risk_lut + (size_t)r_idx[k] * W;
                const int64_t* ql = a.req_lut + (size_t)q_idx[k] * W;
                for (int64_t w = 0; w < W; ++w) {
                    if (st) arow[a.dim_tenant * W + w] = tl[w];
                    if (so) arow[a.dim_topic * W + w] = ol[w];
                    if (sr) arow[a.dim_risk * W + w] = has_risk ? rl[w] : 0;
                    if (sq) lrow[a.all_requires * W + w] = has_req ? ql[w] : 0;
                }
            }
        }
        // phase 3: per-step payload stamp (word 0 of each row)
        if (a.payload != nullptr) {
            int32_t* p = a.payload + (size_t)b0 * a.payload_words;
            for (int k = 0; k < n; ++k, p += a.payload_words) *p = stamp;
        }
    }
}

static void encode_range_base(const EncodeJob& a, int64_t i0, int64_t i1) {
    encode_range_impl(a, i0, i1);
}

// ISA levels: 0 baseline, 1 AVX2, 2 AVX-512 (F+DQ+VL: 64-bit vector multiply)
#if defined(__x86_64__) && (defined(__GNUC__) || defined(__clang__)) && \
    !defined(__HIP_DEVICE_COMPILE__)
#define CORDUM_ENC_MULTIVERSION 1
__attribute__((target("avx2"))) static void encode_range_avx2(
    const EncodeJob& a, int64_t i0, int64_t i1) {
    encode_range_impl(a, i0, i1);
}
__attribute__((target("avx512f,avx512dq,avx512vl"))) static void encode_range_avx512(
    const EncodeJob& a, int64_t i0, int64_t i1) {
    encode_range_impl(a, i0, i1);
}
static inline int max_isa_level() {
    __builtin_cpu_init();
    if (__builtin_cpu_supports("avx512f") && __builtin_cpu_supports("avx512dq") &&
        __builtin_cpu_supports("avx512vl"))
        return 2;
    if (__builtin_cpu_supports("avx2")) return 1;
    return 0;
}
#else
static inline int max_isa_level() { return 0; }
#endif

// isa_cap < 0: best the CPU has; otherwise min(isa_cap, best)
static inline void encode_range(const EncodeJob& a, int64_t i0, int64_t i1, int isa_cap) {
    int level = max_isa_level();
    if (isa_cap >= 0 && isa_cap < level) level = isa_cap;
#ifdef CORDUM_ENC_MULTIVERSION
    if (level >= 2) return encode_range_avx512(a, i0, i1);
    if (level == 1) return encode_range_avx2(a, i0, i1);
#endif
    (void)level;
    encode_range_base(a, i0, i1);
}

// Whole batch. threads <= 1: serial on the caller. threads >= 2: the upper
// half runs on one helper thread this call creates and joins (split on a
// block boundary so both halves hash whole blocks).
static inline void encode_batch(const EncodeJob& a, int threads, int isa_cap) {
    const int64_t nblocks = (a.B + kBlock - 1) / kBlock;
    if (threads < 2 || nblocks < 2) {
        encode_range(a, 0, a.B, isa_cap);
        return;
    }
    const int64_t mid = (nblocks / 2) * kBlock;
    std::thread helper([&a, mid, isa_cap] { encode_range(a, mid, a.B, isa_cap); });
    encode_range(a, 0, mid, isa_cap);
    helper.join();
}

}  // namespace cordum_enc
