// Stand-alone check of the compact mode of cordum_amd/ops/hip/synthetic_encode.h
// (rows of L columns, one per dimension the compiled policy reads; a negative
// column = that dim is not stored), the counterpart of encode_check.cpp. Meant
// to be built with -fsanitize=address,undefined and run on the CPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -pthread \
//       -Icordum_amd/ops/hip tests/native/encode_compact_check.cpp \
//       -o encode_compact_check
// The cols array is a heap block of exactly B*L words (none at all for L = 0),
// so a store past a row, or any store where no dim has a column, is an ASan
// report. Values are compared against a plain serial loop that computes each
// job's four words from the hash chain and places them by column.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "synthetic_encode.h"

using cordum_enc::EncodeJob;

struct Columns {
    int L;
    int tenant, topic, risk, requires_;  // column, or -1: not stored
};

static void serial_reference(int64_t* cols, const Columns& c, int64_t B, int64_t V,
                             uint64_t seed, uint64_t step, const int64_t* const luts[4]) {
    const uint64_t base = cordum_enc::batch_base(seed, step);
    for (int64_t i = 0; i < B; ++i) {
        const uint64_t h0 = cordum_enc::splitmix64(base ^ (uint64_t)i);
        const uint64_t h1 = cordum_enc::splitmix64(h0);
        const uint64_t h2 = cordum_enc::splitmix64(h1);
        const uint64_t idx[4] = {
            ((h0 & 0xffffffffull) * (uint64_t)V) >> 32, ((h0 >> 32) * (uint64_t)V) >> 32,
            ((h1 & 0xffffffffull) * (uint64_t)V) >> 32, ((h1 >> 32) * (uint64_t)V) >> 32};
        const int64_t word[4] = {
            luts[0][idx[0]], luts[1][idx[1]],
            (uint32_t)h2 < cordum_enc::kRiskCut ? luts[2][idx[2]] : 0,
            (uint32_t)(h2 >> 32) < cordum_enc::kReqCut ? luts[3][idx[3]] : 0};
        const int col[4] = {c.tenant, c.topic, c.risk, c.requires_};
        for (int k = 0; k < 4; ++k)
            if (col[k] >= 0) cols[i * c.L + col[k]] = word[k];
    }
}

static int check(int64_t B, const Columns& c, uint64_t step, int threads, int isa, int64_t pw) {
    const int64_t V = 48;
    std::vector<int64_t> luts[4];
    uint64_t x = 0x4321 + (uint64_t)c.L;
    for (auto& l : luts) {
        l.resize((size_t)V);
        for (auto& e : l) e = (int64_t)(x = cordum_enc::splitmix64(x));
    }
    const int64_t* const lp[4] = {luts[0].data(), luts[1].data(), luts[2].data(),
                                  luts[3].data()};
    const int64_t kFill = 0x5A5A5A5A;
    // malloc, not vector: exact-size blocks with redzones on both sides
    const size_t n = (size_t)(B * c.L);
    int64_t* cols = n ? (int64_t*)malloc(n * 8) : nullptr;
    int64_t* rcols = n ? (int64_t*)malloc(n * 8) : nullptr;
    int32_t* payload = (int32_t*)malloc((size_t)(B * pw) * 4);
    for (size_t i = 0; i < n; ++i) cols[i] = rcols[i] = kFill;
    for (int64_t i = 0; i < B * pw; ++i) payload[i] = (int32_t)(i * 2654435761u);

    serial_reference(rcols, c, B, V, 11, step, lp);

    EncodeJob a{};
    a.any = cols; a.all = cols;
    a.any_stride = c.L; a.all_stride = c.L;
    a.tenant_lut = lp[0]; a.topic_lut = lp[1]; a.risk_lut = lp[2]; a.req_lut = lp[3];
    a.B = B; a.W = 1; a.V = V;
    a.seed = 11; a.step = step;
    a.dim_tenant = c.tenant; a.dim_topic = c.topic; a.dim_risk = c.risk;
    a.all_requires = c.requires_;
    a.payload = payload; a.payload_words = pw;
    cordum_enc::encode_batch(a, threads, isa);

    int bad = 0;
    if (n && memcmp(cols, rcols, n * 8) != 0) bad |= 1;
    for (int64_t i = 0; i < B * pw; ++i) {
        const int32_t want = (i % pw == 0) ? (int32_t)(uint32_t)step
                                           : (int32_t)(i * 2654435761u);
        if (payload[i] != want) { bad |= 4; break; }
    }
    if (bad)
        printf("MISMATCH mask=%d B=%lld L=%d cols=%d,%d,%d,%d step=%llu threads=%d isa=%d "
               "pw=%lld\n", bad, (long long)B, c.L, c.tenant, c.topic, c.risk, c.requires_,
               (unsigned long long)step, threads, isa, (long long)pw);
    free(cols); free(rcols); free(payload);
    return bad ? 1 : 0;
}

int main() {
    const int64_t Bs[] = {1, 63, 64, 65, 127, 128, 129, 1000, 4113};
    const uint64_t steps[] = {0, 7, (1ull << 32) + 3};
    // the synthetic four alone; among other columns (sentinels between them
    // must stay); one of the four not stored; a single column; none (L = 0)
    const Columns layouts[] = {
        {4, 0, 1, 2, 3},
        {9, 0, 1, 6, 7},
        {4, 0, 1, -1, 3},
        {3, -1, 2, 0, -1},
        {1, -1, 0, -1, -1},
        {0, -1, -1, -1, -1},
    };
    const int top = cordum_enc::max_isa_level();
    int failures = 0, cases = 0;
    for (int64_t B : Bs)
        for (const Columns& c : layouts)
            for (uint64_t step : steps)
                for (int threads = 1; threads <= 2; ++threads)
                    for (int isa = 0; isa <= top; ++isa)
                        for (int64_t pw : {(int64_t)1, (int64_t)5}) {
                            failures += check(B, c, step, threads, isa, pw);
                            ++cases;
                        }
    printf("isa level %d, %d cases, %d failures\n", top, cases, failures);
    if (failures) return 1;
    printf("encode_compact_check ok\n");
    return 0;
}
