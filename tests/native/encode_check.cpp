// Stand-alone check of cordum_amd/ops/hip/synthetic_encode.h, meant to be
// built with -fsanitize=address,undefined and run on the CPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -pthread \
//       -Icordum_amd/ops/hip tests/native/encode_check.cpp -o encode_check
// Every buffer is a heap allocation of exactly the size the encoder may
// touch, so a store past a row, a LUT read past V or a stamp past the
// payload ring is an ASan report. Values are compared against the plain
// serial loop (the shape of ext.synthetic_fresh).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "synthetic_encode.h"

using cordum_enc::EncodeJob;

static void serial_reference(const EncodeJob& a) {
    const uint64_t base = cordum_enc::batch_base(a.seed, a.step);
    const uint64_t v = (uint64_t)a.V;
    for (int64_t i = 0; i < a.B; ++i) {
        const uint64_t h0 = cordum_enc::splitmix64(base ^ (uint64_t)i);
        const uint64_t h1 = cordum_enc::splitmix64(h0);
        const uint64_t h2 = cordum_enc::splitmix64(h1);
        const int64_t t = (int64_t)(((h0 & 0xffffffffull) * v) >> 32);
        const int64_t o = (int64_t)(((h0 >> 32) * v) >> 32);
        const int64_t r = (int64_t)(((h1 & 0xffffffffull) * v) >> 32);
        const int64_t q = (int64_t)(((h1 >> 32) * v) >> 32);
        const bool has_risk = (uint32_t)h2 < cordum_enc::kRiskCut;
        const bool has_req = (uint32_t)(h2 >> 32) < cordum_enc::kReqCut;
        int64_t* arow = a.any + (size_t)i * 7 * a.W;
        int64_t* lrow = a.all + (size_t)i * 2 * a.W;
        for (int64_t w = 0; w < a.W; ++w) {
            arow[a.dim_tenant * a.W + w] = a.tenant_lut[t * a.W + w];
            arow[a.dim_topic * a.W + w] = a.topic_lut[o * a.W + w];
            arow[a.dim_risk * a.W + w] = has_risk ? a.risk_lut[r * a.W + w] : 0;
            lrow[a.all_requires * a.W + w] = has_req ? a.req_lut[q * a.W + w] : 0;
        }
    }
}

static int check(int64_t B, int64_t W, uint64_t step, int threads, int isa, int64_t pw) {
    const int64_t V = 48;
    std::vector<int64_t> luts[4];
    uint64_t x = 0x1234 + (uint64_t)W;
    for (auto& l : luts) {
        l.resize((size_t)(V * W));
        for (auto& e : l) e = (int64_t)(x = cordum_enc::splitmix64(x));
    }
    const int64_t kFill = 0x5A5A5A5A;
    // malloc, not vector: exact-size blocks with redzones on both sides
    const size_t n_any = (size_t)(B * 7 * W), n_all = (size_t)(B * 2 * W);
    int64_t* any = (int64_t*)malloc(n_any * 8);
    int64_t* all = (int64_t*)malloc(n_all * 8);
    int64_t* rany = (int64_t*)malloc(n_any * 8);
    int64_t* rall = (int64_t*)malloc(n_all * 8);
    int32_t* payload = (int32_t*)malloc((size_t)(B * pw) * 4);
    for (size_t i = 0; i < n_any; ++i) any[i] = rany[i] = kFill;
    for (size_t i = 0; i < n_all; ++i) all[i] = rall[i] = kFill;
    for (int64_t i = 0; i < B * pw; ++i) payload[i] = (int32_t)(i * 2654435761u);

    EncodeJob a{};
    a.tenant_lut = luts[0].data();
    a.topic_lut = luts[1].data();
    a.risk_lut = luts[2].data();
    a.req_lut = luts[3].data();
    a.B = B; a.W = W; a.V = V;
    a.seed = 11; a.step = step;
    a.dim_tenant = 0; a.dim_topic = 1; a.dim_risk = 3; a.all_requires = 0;
    a.payload_words = pw;

    EncodeJob ref = a;
    ref.any = rany; ref.all = rall; ref.payload = nullptr;
    serial_reference(ref);

    a.any = any; a.all = all; a.payload = payload;
    cordum_enc::encode_batch(a, threads, isa);

    int bad = 0;
    if (memcmp(any, rany, n_any * 8) != 0) bad |= 1;
    if (memcmp(all, rall, n_all * 8) != 0) bad |= 2;
    for (int64_t i = 0; i < B * pw; ++i) {
        const int32_t want = (i % pw == 0) ? (int32_t)(uint32_t)step
                                           : (int32_t)(i * 2654435761u);
        if (payload[i] != want) { bad |= 4; break; }
    }
    if (bad)
        printf("MISMATCH mask=%d B=%lld W=%lld step=%llu threads=%d isa=%d pw=%lld\n", bad,
               (long long)B, (long long)W, (unsigned long long)step, threads, isa, (long long)pw);
    free(any); free(all); free(rany); free(rall); free(payload);
    return bad ? 1 : 0;
}

int main() {
    const int64_t Bs[] = {1, 63, 64, 65, 127, 128, 129, 1000, 4113};
    const uint64_t steps[] = {0, 7, (1ull << 32) + 3};
    const int top = cordum_enc::max_isa_level();
    int failures = 0, cases = 0;
    for (int64_t B : Bs)
        for (int64_t W = 1; W <= 2; ++W)
            for (uint64_t step : steps)
                for (int threads = 1; threads <= 2; ++threads)
                    for (int isa = 0; isa <= top; ++isa)
                        for (int64_t pw : {(int64_t)1, (int64_t)5}) {
                            failures += check(B, W, step, threads, isa, pw);
                            ++cases;
                        }
    printf("isa level %d, %d cases, %d failures\n", top, cases, failures);
    if (failures) return 1;
    printf("encode_check ok\n");
    return 0;
}
