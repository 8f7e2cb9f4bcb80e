// CDNA4 (gfx950) kernels for the cordum_amd control plane.
//
// K1 policy_first_match   — batched rule×job policy evaluation
//                           (replaces SafetyPolicy.Evaluate, safety_policy.go:187-294)
// K2 least_loaded_pick    — batched worker scoring + masked argmin
//                           (replaces PickSubject, strategy_least_loaded.go:40-136)
// K4 deadline_scan        — deadline/timeout sweep over the job table
//                           (replaces reconciler.go:88-144 + job_store deadline ZSET)
// K5 apply_transitions    — batched job state transitions with the legality LUT
//                           (replaces job_store.go:249-329 WATCH/tx)
// W  echo_worker          — device worker pool execution (payload touch + result)
//
// Design notes (see /opt/skills/guides/cdna_hip_programming.md):
//  - wave64; blocks of 256 threads; grid-stride where applicable.
//  - policy kernel: one job per thread, rules staged through LDS in chunks by
//    the whole workgroup (rule rows are reused by all 256 threads; LDS
//    staging turns R global reads per thread into R/256 per thread).
//  - first-match across rule chunks uses atomicMin on the output word (the
//    output is initialized to INT_MAX by the host); chunk-level early-out
//    via a workgroup ballot on "all jobs in this block already matched an
//    earlier rule".
//  - scoring kernel: score = active + cpu/100 + gpu/100 packed into a
//    monotonic (score,idx) uint64 key -> deterministic argmin (ties by
//    lowest worker index, matching the host strategy).
//
// Stage bodies: the logic of each tick stage is one __device__
// __forceinline__ function in the "Tick stage bodies" section below
// (worker_key, begin_slot, gate_job = gate_decide + gate_append, the K5 rule
// as apply_one/march_chain, deny_to_dlq, spread_worker/route_pick/
// route_append, echo_row, wave_histogram_add). The per-stage kernels (eager,
// padded and staged ticks) call one body each; the fused kernels compose
// several:
//   tick_prologue = begin_slot + worker_key
//   gate_route    = gate_job + deny_to_dlq + route_pick + route_append
//   tick_finish   = wave_histogram_add + echo_row + march_chain + counter fold
// The wf_* kernels, K1, the K2 scan, the pack kernels and deadline_scan do
// not go through them.
#include <hip/hip_runtime.h>
#include <cstdint>

#define WAVE 64
#define BLOCK 256

// ---------------------------------------------------------------------------
// K1: policy first-match
// ---------------------------------------------------------------------------
// Rule row layout (int64 words, W words per dim):
//   any[7*W] | all[2*W] | mcp_allow[4*W] | mcp_deny[4*W]
// plus per-rule bytes: secrets(int8), mcp_any(u8).
// Job row: any[7*W] | all[2*W] | mcp[4*W], secrets u8, mcp_used u8.

template <int W, int JPT>
__global__ __launch_bounds__(BLOCK) void policy_first_match_kernel(
    const long long* __restrict__ rule_any,   // [R,7,W]
    const long long* __restrict__ rule_all,   // [R,2,W]
    const signed char* __restrict__ rule_secrets, // [R]
    const long long* __restrict__ rule_mcp,   // [R,4,2,W]
    const unsigned char* __restrict__ rule_mcp_any, // [R]
    const long long* __restrict__ job_any,    // [J,7,W]
    const long long* __restrict__ job_all,    // [J,2,W]
    const unsigned char* __restrict__ job_secrets, // [J]
    const long long* __restrict__ job_mcp,    // [J,4,W]
    const unsigned char* __restrict__ job_mcp_used, // [J]
    int* __restrict__ out_first,              // [J], pre-filled INT_MAX
    int R, int J, int rules_per_chunk)
{
    // 2D grid: blockIdx.x tiles jobs (JPT jobs per thread — the rule stream
    // is the traffic bound at large R, and every extra job per block divides
    // it), blockIdx.y tiles the rule range; first-match semantics restored
    // by the atomicMin on the output word.
    const int rule_chunk_begin = blockIdx.y * rules_per_chunk;
    const int rule_chunk_end = min(R, rule_chunk_begin + rules_per_chunk);
    constexpr int ANY_W = 7 * W;
    constexpr int ALL_W = 2 * W;
    constexpr int MCP_W = 4 * W;
    constexpr int ROW = ANY_W + ALL_W + 2 * MCP_W;     // int64 words per rule
    constexpr int CHUNK = 96;                          // rules staged per LDS pass

    __shared__ long long lds_rules[CHUNK * ROW];
    __shared__ signed char lds_secrets[CHUNK];
    __shared__ unsigned char lds_mcp_any[CHUNK];
    __shared__ int block_done;

    int jj[JPT];
    long long jany[JPT][ANY_W], jall[JPT][ALL_W], jmcp[JPT][MCP_W];
    unsigned char jsec[JPT], jused[JPT];
    int best[JPT];
    #pragma unroll
    for (int k = 0; k < JPT; ++k) {
        const int j = (blockIdx.x * JPT + k) * BLOCK + threadIdx.x;
        jj[k] = j;
        best[k] = INT_MAX;
        if (j < J) {
            #pragma unroll
            for (int w = 0; w < ANY_W; ++w) jany[k][w] = job_any[(size_t)j * ANY_W + w];
            #pragma unroll
            for (int w = 0; w < ALL_W; ++w) jall[k][w] = job_all[(size_t)j * ALL_W + w];
            #pragma unroll
            for (int w = 0; w < MCP_W; ++w) jmcp[k][w] = job_mcp[(size_t)j * MCP_W + w];
            jsec[k] = job_secrets[j];
            jused[k] = job_mcp_used[j];
        } else {
            best[k] = INT_MAX - 1;  // dead
        }
    }

    for (int base = rule_chunk_begin; base < rule_chunk_end; base += CHUNK) {
        const int n = min(CHUNK, rule_chunk_end - base);
        for (int i = threadIdx.x; i < n * ROW; i += BLOCK) {
            const int r = i / ROW, w = i % ROW;
            const size_t g = (size_t)(base + r);
            long long v;
            if (w < ANY_W)                 v = rule_any[g * ANY_W + w];
            else if (w < ANY_W + ALL_W)    v = rule_all[g * ALL_W + (w - ANY_W)];
            else                           v = rule_mcp[g * 2 * MCP_W + (w - ANY_W - ALL_W)];
            lds_rules[i] = v;
        }
        for (int i = threadIdx.x; i < n; i += BLOCK) {
            lds_secrets[i] = rule_secrets[base + i];
            lds_mcp_any[i] = rule_mcp_any[base + i];
        }
        __syncthreads();

        #pragma unroll
        for (int k = 0; k < JPT; ++k) {
            // cross-chunk early-skip (atomicMin output is monotonic; a stale
            // read only wastes a scan, never correctness)
            if (best[k] == INT_MAX && base > 0 &&
                __hip_atomic_load(&out_first[jj[k]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < base) {
                best[k] = INT_MAX - 1;
            }
            if (best[k] != INT_MAX) continue;
            for (int r = 0; r < n; ++r) {
                const long long* row = &lds_rules[r * ROW];
                bool ok = true;
                #pragma unroll
                for (int d = 0; d < 7 && ok; ++d) {
                    long long inter = 0, any = 0;
                    #pragma unroll
                    for (int w = 0; w < W; ++w) {
                        const long long rm = row[d * W + w];
                        any |= rm;
                        inter |= rm & jany[k][d * W + w];
                    }
                    ok = (any == 0) | (inter != 0);
                }
                #pragma unroll
                for (int d = 0; d < 2 && ok; ++d) {
                    long long missing = 0;
                    #pragma unroll
                    for (int w = 0; w < W; ++w)
                        missing |= row[ANY_W + d * W + w] & ~jall[k][d * W + w];
                    ok = (missing == 0);
                }
                if (ok) {
                    const signed char rs = lds_secrets[r];
                    ok = (rs < 0) | (rs == (signed char)jsec[k]);
                }
                if (ok && jused[k] && lds_mcp_any[r]) {
                    const long long* allow = &row[ANY_W + ALL_W];
                    const long long* deny = &row[ANY_W + ALL_W + MCP_W];
                    #pragma unroll
                    for (int f = 0; f < 4 && ok; ++f) {
                        long long a = 0, ainter = 0, dinter = 0;
                        #pragma unroll
                        for (int w = 0; w < W; ++w) {
                            a |= allow[f * W + w];
                            ainter |= allow[f * W + w] & jmcp[k][f * W + w];
                            dinter |= deny[f * W + w] & jmcp[k][f * W + w];
                        }
                        ok = (dinter == 0) & ((a == 0) | (ainter != 0));
                    }
                }
                if (ok) { best[k] = base + r; break; }
            }
        }
        __syncthreads();
        // chunk early-out: every live job in this block already matched
        if (threadIdx.x == 0) block_done = 1;
        __syncthreads();
        #pragma unroll
        for (int k = 0; k < JPT; ++k)
            if (best[k] == INT_MAX) block_done = 0;
        __syncthreads();
        if (block_done) break;
    }

    #pragma unroll
    for (int k = 0; k < JPT; ++k)
        if (jj[k] < J && best[k] < INT_MAX - 1) atomicMin(&out_first[jj[k]], best[k]);
}

// ---------------------------------------------------------------------------
// Tick stage bodies
// ---------------------------------------------------------------------------
// Each stage of the control-plane tick is written ONCE here as a
// __device__ __forceinline__ body. The __global__ kernels further down (the
// per-stage ones the eager and padded ticks launch, the *_dyn ones of the
// staged captured tick, and the three fused ones) hold only the index
// arithmetic (which thread or wave owns which entry, the bounds, the
// region-valid test of the padded forms) and call into these, so a change to
// a stage is a change in one place.

// job states (protocol/states.py JobState) the rules below name
#define N_STATES 11
#define STATE_PENDING 1
#define STATE_SCHEDULED 3
#define STATE_FIRST_TERMINAL 6   // SUCCEEDED..DENIED are 6..10
#define STATE_DENIED 10
#define NO_DEADLINE ((long long)0x7fffffffffffffffLL)
__constant__ unsigned char d_transition_lut[N_STATES * N_STATES];

// high word of an overloaded worker's key: sorts after every score, before
// the picker's "no candidate" ~0
#define OVERLOADED_TAG 0xfffffffeu

__device__ __forceinline__ unsigned long long score_key(float score, int widx) {
    // score >= 0 -> float bits are monotonic; tie-break by lowest index
    unsigned int sb = __float_as_uint(score);
    return ((unsigned long long)sb << 32) | (unsigned int)widx;
}

// Worker key: (score, idx) packed into a monotonic u64; an overloaded worker
// gets the OVERLOADED_TAG key so the picker can still distinguish "all
// overloaded" from "no workers". The float expressions stay as written: the
// key bits depend on how the compiler contracts them.
__device__ __forceinline__ unsigned long long worker_key(
    int i, int active, int maxp, float cpu, float gpu)
{
    bool over = false;
    if (maxp > 0 && (float)active / (float)maxp >= 0.9f) over = true;
    if (cpu >= 90.f || gpu >= 90.f) over = true;
    if (over) return ((unsigned long long)OVERLOADED_TAG << 32) | (unsigned int)i;
    const float score = (float)active + cpu * 0.01f + gpu * 0.01f;
    return score_key(score, i);
}

// Tick prologue for grid thread i: every ring slot is re-admitted as PENDING
// (CREATED -> PENDING is the only LUT edge exercised by the old zero_() +
// apply_transitions pair, so write it directly), `first` (if given) is
// primed to the atomicMin identity, and the counter words reset.
__device__ __forceinline__ void begin_slot(
    int i, unsigned char* states, int B, int* counts, int ncounts, int* first)
{
    if (i < B) {
        states[i] = STATE_PENDING;
        if (first != nullptr) first[i] = INT_MAX;
    }
    if (i < ncounts) counts[i] = 0;
}

// wave-aggregated compaction append: one atomicAdd per wave instead of one
// per lane (a single counter word saturates at ~88 atomics/us on this chip —
// MI355X_MICROARCH.md price-list row "dequeue")
__device__ __forceinline__ int wave_append_slot(bool pred, int* counter, int lane) {
    const unsigned long long mask = __ballot(pred);
    const int nactive = __popcll(mask);
    int base = 0;
    const int leader = __ffsll((long long)mask) - 1;
    if (pred && lane == leader) base = atomicAdd(counter, nactive);
    base = __shfl(base, leader, WAVE);
    const int rank = __popcll(mask & ((1ull << lane) - 1ull));
    return pred ? base + rank : -1;
}

// Gate decision of job j: the first-matched rule's decision, default allow.
// No-match is -1 (host-masked) OR anything out of range: the raw INT_MAX
// atomicMin identity when the producer skipped the mask pass (_into variants)
__device__ __forceinline__ signed char gate_decide(
    const int* first, const signed char* decisions, int R, int j)
{
    const int r = first[j];
    return (r >= 0 && r < R) ? decisions[r] : (signed char)1;
}

// Allowed/denied split of a live job into the two compacted lists (whole
// wave calls this; dead lanes pass live=false). Returns "allowed".
__device__ __forceinline__ bool gate_append(
    bool live, signed char d, int j, int lane,
    int* allowed_slots, int* allowed_count, int* denied_slots, int* denied_count)
{
    const bool allowed = live && (d == 1 || d == 5);
    const int apos = wave_append_slot(allowed, allowed_count, lane);
    if (apos >= 0) allowed_slots[apos] = j;
    const bool denied = live && !allowed;
    const int dpos = wave_append_slot(denied, denied_count, lane);
    if (dpos >= 0) denied_slots[dpos] = j;
    return allowed;
}

// The gate for grid thread j of J jobs: decide, record the decision, split.
// Returns "allowed".
__device__ __forceinline__ bool gate_job(
    int j, int J, int lane, const int* first, const signed char* decisions, int R,
    signed char* out_decision,
    int* allowed_slots, int* allowed_count, int* denied_slots, int* denied_count)
{
    const bool live = j < J;
    signed char d = 0;
    if (live) {
        d = gate_decide(first, decisions, R, j);
        out_decision[j] = d;
    }
    return gate_append(live, d, j, lane, allowed_slots, allowed_count,
                       denied_slots, denied_count);
}

// K5 rule, one hop, on a state held in a register (job_store.go:70-82):
// legal per the LUT or nothing happens; attempts increment on entering
// SCHEDULED. Advances `cur` and returns true when the hop is legal.
__device__ __forceinline__ bool transition_hop(
    unsigned char& cur, unsigned char to, int* attempts, int slot)
{
    if (!d_transition_lut[cur * N_STATES + to]) return false;
    if (to == STATE_SCHEDULED && cur != STATE_SCHEDULED) attempts[slot] += 1;
    cur = to;
    return true;
}

// ... and the write-back: terminal states clear the deadline
__device__ __forceinline__ void commit_state(
    unsigned char* states, long long* deadlines, int slot, unsigned char cur)
{
    states[slot] = cur;
    if (cur >= STATE_FIRST_TERMINAL) deadlines[slot] = NO_DEADLINE;
}

// One K5 transition of `slot`; an illegal one writes nothing. `attempts` is
// only touched when `to` is SCHEDULED.
__device__ __forceinline__ bool apply_one(
    unsigned char* states, int* attempts, long long* deadlines, int slot, unsigned char to)
{
    unsigned char cur = states[slot];
    if (!transition_hop(cur, to, attempts, slot)) return false;
    commit_state(states, deadlines, slot, cur);
    return true;
}

// Chained K5: march `slot` through up to 4 states (-1 = unused), LUT-checked
// hop by hop, stopping at the first illegal one; the state reached is
// written back once.
__device__ __forceinline__ void march_chain(
    unsigned char* states, int* attempts, long long* deadlines, int slot,
    const int (&chain)[4])
{
    unsigned char cur = states[slot];
    #pragma unroll
    for (int c = 0; c < 4; ++c) {
        if (chain[c] < 0) break;
        if (!transition_hop(cur, (unsigned char)chain[c], attempts, slot)) break;
    }
    commit_state(states, deadlines, slot, cur);
}

// DENIED transition of a denied job + DLQ ring append (K7: dlq_store.go's
// capped index as an HBM ring with an atomic head). Whole wave calls this.
__device__ __forceinline__ void deny_to_dlq(
    bool denied, int j, int lane, unsigned char* states, long long* deadlines,
    int* dlq_ring, int* dlq_head, int ring_size)
{
    const bool dlq = denied && apply_one(states, nullptr, deadlines, j, STATE_DENIED);
    const int rpos = wave_append_slot(dlq, dlq_head, lane);
    if (rpos >= 0) dlq_ring[rpos % ring_size] = j;
}

// K2c: batch spreading — unconstrained jobs round-robin over the K least
// loaded workers. A frozen-snapshot argmin sends a whole homogeneous batch
// to ONE worker (the reference has the same pathology between heartbeats:
// its scheduler replica piles onto the lowest scorer until the next 10 s
// heartbeat); queue-group fan-in is the intended behavior, and spreading a
// batch across the least-loaded set IS that behavior for a batched tick.
// Constrained jobs (labels / narrowed pool mask) keep their exact scan pick.
// Returns job j's spread worker, or -1 when j keeps its exact pick (it is
// constrained, or every worker is overloaded).
__device__ __forceinline__ int spread_worker(
    int j, const int* order, const int* valid_count,
    const long long* j_poolmask, const long long* j_labels, long long full_mask, int K)
{
    if (j_labels[j] != 0 || j_poolmask[j] != full_mask) return -1;
    const int V = min(*valid_count, K);
    return (V > 0) ? order[j % V] : -1;
}

// Route of job j: the spread if it takes one, else the exact pick (<0 = none)
__device__ __forceinline__ int route_pick(
    int j, const int* pick, const int* order, const int* valid_count,
    const long long* j_poolmask, const long long* j_labels, long long full_mask, int K)
{
    const int s = spread_worker(j, order, valid_count, j_poolmask, j_labels, full_mask, K);
    return s >= 0 ? s : pick[j];
}

// Routable compaction: jobs with a worker (w >= 0) go to the routable list.
// Whole wave calls this; lanes without a job pass w < 0.
__device__ __forceinline__ void route_append(
    int j, int w, int lane, int* routable_slots, int* routable_widx, int* routable_count)
{
    const int pos = wave_append_slot(w >= 0, routable_count, lane);
    if (pos >= 0) {
        routable_slots[pos] = j;
        routable_widx[pos] = w;
    }
}

// Echo worker, one wave per job: lanes stream the payload row, echo it into
// the result row (memory-bound, like the reference's echo worker copying
// ctx -> res through Redis) and wave-reduce a checksum, returned in lane 0.
__device__ __forceinline__ unsigned int echo_row(
    const unsigned int* src, unsigned int* dst, int stride, int lane)
{
    unsigned int acc = 0;
    for (int k = lane; k < stride; k += WAVE) {
        const unsigned int v = src[k];
        dst[k] = v;
        acc += v;
    }
    #pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        acc += __shfl_down(acc, off, WAVE);
    return acc;
}

// Load histogram, wave match-any aggregation: a frozen-snapshot least-loaded
// pick is highly concentrated (often ONE worker for a whole homogeneous
// batch), so per-lane atomics serialize on a single word (~88 atomics/us).
// Group lanes by equal bin and issue one atomicAdd per distinct value.
// Whole wave calls this; lanes without an entry pass live=false.
__device__ __forceinline__ void wave_histogram_add(bool live, int bin, int* hist, int lane)
{
    unsigned long long pending = __ballot(live);
    while (pending) {
        const int leader = __ffsll((long long)pending) - 1;
        const int leader_bin = __shfl(bin, leader, WAVE);
        const unsigned long long same = __ballot(live && bin == leader_bin);
        if (lane == leader) atomicAdd(&hist[leader_bin], __popcll(same));
        pending &= ~same;
    }
}

// ---------------------------------------------------------------------------
// K2: least-loaded worker pick
// ---------------------------------------------------------------------------
// Worker row: pool(int32), active(int32), maxp(int32), cpu(f32), gpu(f32),
// labels_mask(int64). Job row: pool_mask(int64 over pool vocab), required
// labels mask(int64), preferred_worker(int32, -1 none).
// Output per job: packed pick int32 (-1 no_workers, -2 overloaded) .

// per-worker tick-invariant precompute of the keys
__global__ __launch_bounds__(BLOCK) void worker_precompute_kernel(
    const int* __restrict__ w_pool,        // [W]
    const int* __restrict__ w_active,      // [W]
    const int* __restrict__ w_maxp,        // [W]
    const float* __restrict__ w_cpu,       // [W]
    const float* __restrict__ w_gpu,       // [W]
    unsigned long long* __restrict__ w_key, // [W] out: (score,idx) or flags
    int NW)
{
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= NW) return;
    w_key[i] = worker_key(i, w_active[i], w_maxp[i], w_cpu[i], w_gpu[i]);
}

__global__ __launch_bounds__(BLOCK) void least_loaded_pick_kernel(
    const int* __restrict__ w_pool,         // [W]
    const unsigned long long* __restrict__ w_key, // [W] from precompute
    const long long* __restrict__ w_labels, // [W]
    const long long* __restrict__ j_poolmask, // [J]
    const long long* __restrict__ j_labels,   // [J] required labels
    int* __restrict__ out_pick,             // [J]
    int NW, int NJ,
    const int* __restrict__ valid_count,    // [1] or nullptr: skip gate
    long long full_mask)
{
    // K2c short-circuit: when any worker is non-overloaded, unconstrained
    // jobs take the spread (round-robin over the sorted order) in the
    // compaction kernel — their exact scan pick is dead work. The full
    // 1000-worker scan was 15.5% of the tick for picks that were
    // overwritten (profiles/r15_bench_ktrace_stats.txt). -1 here matches
    // the all-overloaded scan outcome (-2): both are "no direct route".
    // (block-uniform check: the scan below has __syncthreads() barriers
    // shared by the block's 4 waves, so only a whole-block skip is legal)
    if (valid_count != nullptr && *valid_count > 0) {
        const int jb = blockIdx.x * (BLOCK / WAVE);
        bool all_skip = true;
        for (int k = 0; k < BLOCK / WAVE; ++k) {
            const int jj = jb + k;
            if (jj < NJ && (j_labels[jj] != 0 || j_poolmask[jj] != full_mask)) {
                all_skip = false;
                break;
            }
        }
        if (all_skip) {
            const int jj = jb + threadIdx.x / WAVE;
            if (jj < NJ && threadIdx.x % WAVE == 0) out_pick[jj] = -1;
            return;
        }
    }
    // one WAVE per job: 64 lanes stride the worker table (staged through LDS
    // once per workgroup, shared by the 4 waves), then a wave min-reduce.
    constexpr int WCHUNK = 1024;
    __shared__ unsigned long long s_key[WCHUNK];
    __shared__ long long s_labels[WCHUNK];
    __shared__ int s_pool[WCHUNK];

    const int wave = threadIdx.x / WAVE;           // 0..3
    const int lane = threadIdx.x % WAVE;
    const int j = blockIdx.x * (BLOCK / WAVE) + wave;

    long long pool_mask = 0, req_labels = 0;
    if (j < NJ) {
        pool_mask = j_poolmask[j];
        req_labels = j_labels[j];
    }

    unsigned long long best = ~0ull;
    int overloaded = 0, total = 0;

    for (int base = 0; base < NW; base += WCHUNK) {
        const int n = min(WCHUNK, NW - base);
        for (int i = threadIdx.x; i < n; i += BLOCK) {
            s_key[i] = w_key[base + i];
            s_labels[i] = w_labels[base + i];
            s_pool[i] = w_pool[base + i];
        }
        __syncthreads();
        if (j < NJ) {
            for (int i = lane; i < n; i += WAVE) {
                const int pool = s_pool[i];
                if (pool < 0 || pool >= 64) continue;
                if (!((pool_mask >> pool) & 1)) continue;
                if (req_labels & ~s_labels[i]) continue;
                ++total;
                const unsigned long long key = s_key[i];
                if ((unsigned int)(key >> 32) == OVERLOADED_TAG) { ++overloaded; continue; }
                if (key < best) best = key;
            }
        }
        __syncthreads();
    }

    // wave reductions (64-lane shuffles)
    #pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long other = __shfl_down(best, off, WAVE);
        if (other < best) best = other;
        overloaded += __shfl_down(overloaded, off, WAVE);
        total += __shfl_down(total, off, WAVE);
    }
    if (lane == 0 && j < NJ) {
        if (best != ~0ull) out_pick[j] = (int)(best & 0xffffffffu);
        else if (total > 0 && overloaded == total) out_pick[j] = -2;
        else out_pick[j] = -1;
    }
}

// K2c spread applied in place over the exact picks (spread_worker)
__global__ __launch_bounds__(BLOCK) void spread_pick_kernel(
    const int* __restrict__ order,        // [NW] worker idx sorted by key asc
    const int* __restrict__ valid_count,  // [1] non-overloaded workers
    const long long* __restrict__ j_poolmask,
    const long long* __restrict__ j_labels,
    long long full_mask,
    int* __restrict__ pick,               // in-out
    int NJ, int K)
{
    const int j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= NJ) return;
    const int s = spread_worker(j, order, valid_count, j_poolmask, j_labels, full_mask, K);
    if (s >= 0) pick[j] = s;
}

// ---------------------------------------------------------------------------
// K5: batched state transitions with legality LUT (apply_one)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void apply_transitions_kernel(
    unsigned char* __restrict__ states,     // [N] job table states
    int* __restrict__ attempts,             // [N]
    const int* __restrict__ slots,          // [B] job slots to transition
    const unsigned char* __restrict__ to_states, // [B] target states
    unsigned char* __restrict__ ok_out,     // [B] 1 = applied
    long long* __restrict__ deadlines,      // [N] cleared on terminal
    int B)
{
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= B) return;
    ok_out[i] = apply_one(states, attempts, deadlines, slots[i], to_states[i]);
}

// K7: DLQ ring append — denied/failed slots into a capped device ring
// (dlq_store.go's capped index as an HBM ring with an atomic head)
__global__ __launch_bounds__(BLOCK) void dlq_ring_append_kernel(
    const int* __restrict__ slots,     // [<=cap]
    const int* __restrict__ count,     // [1]
    int* __restrict__ ring,            // [ring_size]
    int* __restrict__ head,            // [1] monotonically increasing
    int ring_size)
{
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    const int lane = threadIdx.x % WAVE;
    const bool live = i < *count;
    const int pos = wave_append_slot(live, head, lane);
    if (pos >= 0) ring[pos % ring_size] = live ? slots[i] : -1;
}

// ---------------------------------------------------------------------------
// Row-scan helpers of the run/step tables (K3, K3-WF)
// ---------------------------------------------------------------------------
// A run is one row of 64 steps; the step states are one byte each, 64 bytes
// per row. The row-scan kernels (wf_journal, wf_settle, wf_cond_eval,
// wf_hold_scan) give a row 4 lanes: lane q of row r owns steps 16q .. 16q+15,
// which are one 16-byte load at r*64 + q*16, so a wave covers 16 rows, a block
// 64, and the grid is ceil(NR*4 / BLOCK). The four lanes of a row are
// neighbours (lanes 4k .. 4k+3 of a wave). A lane keeps its 16 bytes as four
// words, step 16q+j in byte j&3 of word j>>2, works on 16-bit masks with bit j
// for step 16q+j, and stores the 16 bytes back, as one store, only if one
// changed. Per-block counters: the waves' totals are summed through LDS and
// thread 0 adds them, one atomic per counter and block, not per wave: when
// most waves of a large table have something to add, adds to one word are
// served one after the other.
struct wf_bytes16 { unsigned w[4]; };
struct wf_row_lane { int r, q; size_t off; };       // row, quarter, byte offset of the 16

__device__ __forceinline__ wf_row_lane wf_row_coords() {
    const int t = blockIdx.x * BLOCK + threadIdx.x;
    return {t >> 2, t & 3, (size_t)(t >> 2) * 64 + (size_t)(t & 3) * 16};
}
__device__ __forceinline__ wf_bytes16 load16(const unsigned char* p) {
    const uint4 v = *reinterpret_cast<const uint4*>(p);
    return {{v.x, v.y, v.z, v.w}};
}
__device__ __forceinline__ unsigned byte16(const wf_bytes16& b, int j) {
    return (b.w[j >> 2] >> ((j & 3) * 8)) & 0xffu;
}
// bit j: pred(byte j)
template <class Pred>
__device__ __forceinline__ unsigned mask16(const wf_bytes16& b, Pred pred) {
    unsigned m = 0u;
#pragma unroll
    for (int j = 0; j < 16; ++j) m |= (unsigned)pred(byte16(b, j)) << j;
    return m;
}
// bit j: byte j == value
__device__ __forceinline__ unsigned match16(const wf_bytes16& b, unsigned value) {
    return mask16(b, [=](unsigned x) { return x == value; });
}
// bit j: byte j of a != byte j of b
__device__ __forceinline__ unsigned differ16(const wf_bytes16& a, const wf_bytes16& b) {
    const wf_bytes16 x = {{a.w[0] ^ b.w[0], a.w[1] ^ b.w[1], a.w[2] ^ b.w[2], a.w[3] ^ b.w[3]}};
    return mask16(x, [](unsigned d) { return d != 0u; });
}
// j may be a run-time value: every word is indexed by a constant and the one
// that holds the byte is selected, so the words stay in registers
__device__ __forceinline__ void set_byte(wf_bytes16& b, int j, unsigned value) {
    const int sft = (j & 3) * 8, k = j >> 2;
    const unsigned keep = ~(0xffu << sft), v = value << sft;
    b.w[0] = k == 0 ? (b.w[0] & keep) | v : b.w[0];
    b.w[1] = k == 1 ? (b.w[1] & keep) | v : b.w[1];
    b.w[2] = k == 2 ? (b.w[2] & keep) | v : b.w[2];
    b.w[3] = k == 3 ? (b.w[3] & keep) | v : b.w[3];
}
// one 16-byte store, only if a byte changed (or `always`)
__device__ __forceinline__ void store16_if_changed(unsigned char* p, const wf_bytes16& now,
                                                   const wf_bytes16& old, bool always = false) {
    if (always || now.w[0] != old.w[0] || now.w[1] != old.w[1] || now.w[2] != old.w[2]
        || now.w[3] != old.w[3])
        *reinterpret_cast<uint4*>(p) = make_uint4(now.w[0], now.w[1], now.w[2], now.w[3]);
}
// OR over the four lanes of a row, the result in all four
__device__ __forceinline__ unsigned long long quad_or(unsigned long long x) {
    x |= __shfl_xor(x, 1, WAVE);
    return x | __shfl_xor(x, 2, WAVE);
}
// sum over the wave, the result in every lane
template <typename T>
__device__ __forceinline__ T wave_sum(T x) {
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) x += __shfl_xor(x, d, WAVE);
    return x;
}
// inclusive prefix sum over the wave
__device__ __forceinline__ int wave_prefix_sum(int x, int lane) {
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
        const int v = __shfl_up(x, d, WAVE);
        if (lane >= d) x += v;
    }
    return x;
}
// Block sums of wave totals: v[k] is wave-uniform on entry and the sum over
// the block's waves in thread 0 on return (no other thread may use it). It
// holds the block's barrier, so every thread of the block must get here.
template <typename T, int N>
__device__ __forceinline__ void block_sum(T (&v)[N]) {
    __shared__ T part[N][BLOCK / WAVE];
    if (threadIdx.x % WAVE == 0)
        for (int k = 0; k < N; ++k) part[k][threadIdx.x / WAVE] = v[k];
    __syncthreads();
    if (threadIdx.x == 0)
        for (int k = 0; k < N; ++k) v[k] = part[k][0] + part[k][1] + part[k][2] + part[k][3];
}
template <typename T>
__device__ __forceinline__ T block_sum(T wave_total) {
    T v[1] = {wave_total};
    block_sum(v);
    return v[0];
}
// Appends (run, step) for every set bit of a per-lane 64-step mask to a counted
// list, one bit per lane and pass; entries past cap are counted, not written.
__device__ __forceinline__ void wave_append_steps(
    long long mask, int run, int lane, int* runs, int* steps, int* count, int cap) {
    while (__any(mask != 0)) {
        int step = -1;
        if (mask != 0) { step = __ffsll(mask) - 1; mask &= mask - 1; }
        const int pos = wave_append_slot(step >= 0, count, lane);
        if (pos >= 0 && pos < cap) { runs[pos] = run; steps[pos] = step; }
    }
}

// ---------------------------------------------------------------------------
// K3: run/step readiness sweep over HBM-resident run state
// ---------------------------------------------------------------------------
// Batched equivalent of scheduleReady's dependency gate (workflow/engine.go
// :453-827, depsSatisfied :1231-1242) for runs with <= 64 steps: per run,
// step s is dispatchable when
//   step_state[s] == PENDING(0)  AND  deps_mask[s] subset-of succeeded_mask
// where succeeded_mask bit t = (step_state[t] == SUCCEEDED). Emits a
// compacted (run, step) dispatch list. One thread per run; 64-step bitmask
// per run row (larger workflows stay on the host path).
#define STEP_PENDING_C 0
#define STEP_SUCCEEDED_C 3

__global__ __launch_bounds__(BLOCK) void run_readiness_kernel(
    const unsigned char* __restrict__ step_state, // [NR][64]
    const long long* __restrict__ deps_mask,      // [NR][64]
    const unsigned char* __restrict__ n_steps,    // [NR]
    const unsigned char* __restrict__ run_active, // [NR] 1 = pending/running
    long long* __restrict__ ready_mask_out,       // [NR]
    int* __restrict__ dispatch_runs,              // [cap]
    int* __restrict__ dispatch_steps,             // [cap]
    int* __restrict__ dispatch_count,             // [1]
    int NR, int cap)
{
    const int run = blockIdx.x * BLOCK + threadIdx.x;
    const int lane = threadIdx.x % WAVE;
    long long ready = 0;
    int ns = 0;
    if (run < NR && run_active[run]) {
        ns = n_steps[run];
        const unsigned char* st = &step_state[(size_t)run * 64];
        unsigned long long succeeded = 0;
        #pragma unroll 8
        for (int t = 0; t < ns; ++t)
            succeeded |= (unsigned long long)(st[t] == STEP_SUCCEEDED_C) << t;
        const long long* dm = &deps_mask[(size_t)run * 64];
        for (int s = 0; s < ns; ++s) {
            if (st[s] != STEP_PENDING_C) continue;
            const unsigned long long need = (unsigned long long)dm[s];
            if ((need & ~succeeded) == 0) ready |= 1ll << s;
        }
    }
    if (run < NR) ready_mask_out[run] = ready;
    wave_append_steps(ready, run, lane, dispatch_runs, dispatch_steps, dispatch_count, cap);
}

// ---------------------------------------------------------------------------
// K3-WF: device-resident workflow engine tick (config #3)
// ---------------------------------------------------------------------------
// Batched equivalent of the per-run scheduleReady walk + HandleJobResult +
// updateRunStatus loop (workflow/engine.go:453-827, :1524-1560, :1623-1699)
// over HBM-resident run tables. Step kinds: WORKER (1 child job), FOR_EACH
// (fanout_n children, aggregated like engine.go:1623-1645), APPROVAL
// (WAITING hold until a host grant — the human-in-the-loop hop stays on the
// host, like gateway.go:3553), CONDITION (pre-evaluated bit -> SUCCEEDED or
// SKIPPED), DELAY (next_ready tick gate). Failed children retry with
// exponential tick backoff up to max_retries (computeBackoff analog), then
// the step FAILs and the run FAILs (failure blocks downstream,
// depsSatisfied :1231-1242 — SKIPPED satisfies, FAILED never does).
#define WFS_PENDING 0
#define WFS_DISPATCHED 1
#define WFS_WAITING 2
#define WFS_SUCCEEDED 3
#define WFS_FAILED 4
#define WFS_SKIPPED 5
#define WFK_WORKER 0
#define WFK_FOR_EACH 1
#define WFK_APPROVAL 2
#define WFK_CONDITION 3
#define WFK_DELAY 4

__global__ __launch_bounds__(BLOCK) void wf_sweep_kernel(
    unsigned char* __restrict__ step_state,   // [NR*64]
    const long long* __restrict__ deps_mask,  // [NR*64]
    const unsigned char* __restrict__ n_steps,// [NR]
    const unsigned char* __restrict__ run_active, // [NR]
    const unsigned char* __restrict__ step_kind,  // [NR*64]
    const long long* __restrict__ cond_bits,  // [NR] bit s = condition value
    const int* __restrict__ next_ready,       // [NR*64] tick gate
    const int* __restrict__ tick_p,           // [1] device tick counter
    int* __restrict__ disp_runs,              // [cap] WORKER/FOR_EACH to expand
    int* __restrict__ disp_steps,             // [cap]
    int* __restrict__ disp_count,             // [1]
    int* __restrict__ appr_runs,              // [acap] fresh WAITING approvals
    int* __restrict__ appr_steps,             // [acap]
    int* __restrict__ appr_count,             // [1]
    int NR, int cap, int acap)
{
    const int run = blockIdx.x * BLOCK + threadIdx.x;
    const int lane = threadIdx.x % WAVE;
    const int tick = *tick_p;
    long long disp = 0, appr = 0;
    if (run < NR && run_active[run]) {
        const int ns = n_steps[run];
        unsigned char* st = &step_state[(size_t)run * 64];
        unsigned long long satisfied = 0;
        for (int t = 0; t < ns; ++t) {
            const unsigned char s = st[t];
            satisfied |= (unsigned long long)(s == WFS_SUCCEEDED || s == WFS_SKIPPED) << t;
        }
        const long long* dm = &deps_mask[(size_t)run * 64];
        const long long cb = cond_bits[run];
        for (int s = 0; s < ns; ++s) {
            if (st[s] != WFS_PENDING) continue;
            if (((unsigned long long)dm[s] & ~satisfied) != 0) continue;
            if (next_ready[(size_t)run * 64 + s] > tick) continue;
            switch (step_kind[(size_t)run * 64 + s]) {
            case WFK_WORKER:
            case WFK_FOR_EACH:
                disp |= 1ll << s;
                break;
            case WFK_APPROVAL:
                st[s] = WFS_WAITING;   // held for the host-side grant
                appr |= 1ll << s;
                break;
            case WFK_CONDITION:
                st[s] = ((cb >> s) & 1) ? WFS_SUCCEEDED : WFS_SKIPPED;
                break;
            case WFK_DELAY:            // gate already passed
                st[s] = WFS_SUCCEEDED;
                break;
            }
        }
    }
    wave_append_steps(disp, run, lane, disp_runs, disp_steps, disp_count, cap);
    wave_append_steps(appr, run, lane, appr_runs, appr_steps, appr_count, acap);
}

// for_each expansion: one wave per dispatch entry; all-or-nothing child-slot
// reservation in the child arena (full arena -> step stays PENDING and the
// next sweep retries, natural backpressure like max_parallel windowing)
__global__ __launch_bounds__(BLOCK) void wf_expand_kernel(
    const int* __restrict__ disp_runs,
    const int* __restrict__ disp_steps,
    const int* __restrict__ disp_count,
    unsigned char* __restrict__ step_state,   // [NR*64]
    int* __restrict__ children_todo,          // [NR*64] children left to emit
    int* __restrict__ children_out,           // [NR*64] in flight
    const int* __restrict__ max_parallel,     // [NR*64] 0 = unlimited
    int* __restrict__ child_tag,              // [CB] run*64+step
    int* __restrict__ child_seq,              // [CB] per-step emission ordinal
    int* __restrict__ child_widx,             // [CB] global worker pick
    int* __restrict__ child_count,            // [1]
    int* __restrict__ children_emitted,       // [NR*64] monotone ordinal source
    int* __restrict__ dispatch_tick,          // [NR*64] stamped for K4-WF
    const int* __restrict__ tick_p,           // [1]
    const int* __restrict__ order,            // [NWG] spread order (K2c)
    const int* __restrict__ valid_count,      // [1]
    int disp_cap, int CB)
{
    const int e = (blockIdx.x * BLOCK + threadIdx.x) / WAVE;
    const int lane = threadIdx.x % WAVE;
    if (e >= min(*disp_count, disp_cap)) return;
    const int run = disp_runs[e];
    const int step = disp_steps[e];
    const size_t rs = (size_t)run * 64 + step;
    int base = 0, todo = 0, seq0 = 0;
    if (lane == 0) {
        todo = children_todo[rs];
        // for_each max_parallel windowing (dataflow_test.go:71 semantics):
        // emit only up to the window; the commit pass re-opens the step as
        // soon as in-flight drops below the window
        const int maxp = max_parallel[rs];
        if (maxp > 0) {
            const int room = maxp - children_out[rs];
            if (room < todo) todo = room > 0 ? room : 0;
        }
        // monotone per-step emission counter: a deterministic per-child
        // ordinal stream identical on every backend regardless of atomic
        // packing order (retried children get FRESH ordinals)
        seq0 = children_emitted[rs];
        if (todo > CB) {
            // can never fit: leave the counter alone, so the entry cannot
            // push the ones that do fit out of the arena
            todo = -1;
        } else if (todo > 0) {
            base = atomicAdd(child_count, todo);
            if (base + todo > CB) {
                // arena full: roll back, retry later. A failed add leaves
                // the counter above CB, so nothing is granted until it is
                // lowered, and the lowest failed base is the end of the
                // granted ranges: atomicMin restores exactly that. (Taking
                // only the own todo back, as atomicSub did, kept the other
                // failed adds in the counter, and the next grant reserved a
                // range past the final count, with a hole below it.)
                atomicMin(child_count, base);
                todo = -1;
            } else {
                step_state[rs] = WFS_DISPATCHED;
                children_out[rs] += todo;
                children_emitted[rs] += todo;
                children_todo[rs] -= todo;
                dispatch_tick[rs] = *tick_p;
            }
        } else if (children_out[rs] > 0) {
            // window full: mark DISPATCHED so the sweep stops re-emitting
            // until the commit pass re-opens it
            step_state[rs] = WFS_DISPATCHED;
        }
    }
    base = __shfl(base, 0, WAVE);
    todo = __shfl(todo, 0, WAVE);
    seq0 = __shfl(seq0, 0, WAVE);
    if (todo <= 0) return;
    const int tag = run * 64 + step;
    const int V = max(1, *valid_count);
    for (int k = lane; k < todo; k += WAVE) {
        child_tag[base + k] = tag;
        child_seq[base + k] = seq0 + k;
        // spread: children are unconstrained -> round-robin the least-loaded
        // order (K2c semantics, deterministic)
        child_widx[base + k] = order[(base + k) % min(V, 1024)];
    }
}

// deterministic per-entry failure injection (config #5 retry waves): a
// splitmix-style hash of (tag, tick, arena position) -> fail if < fail_ppt
// per mille. The CPU oracle mirrors this bit-for-bit.
__device__ __forceinline__ unsigned int wf_mix(unsigned int x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

// apply child results over the packed send segments (the owner rank's view
// of what it dispatched this tick; echo workers are deterministic-success,
// failures are injected by a hash of the child's (tag, emission ordinal) —
// independent of packing order, so every backend agrees). Flagged entries
// are redeliveries whose tag/seq live in the rq_prev carries.
// One body for wf_apply and wf_apply_out (device conditions): OUT only adds
// the step-output accumulation, so the counters of the two cannot drift.
template <bool OUT>
__device__ __forceinline__ void wf_apply_one(
    const int i,
    const int* __restrict__ send_slots, const int* __restrict__ send_cnt,
    const int* __restrict__ child_tag, const int* __restrict__ child_seq,
    const int* __restrict__ rq_prev_tag, const int* __restrict__ rq_prev_seq,
    int* __restrict__ children_done, int* __restrict__ children_fail,
    int* __restrict__ children_out,
    const unsigned int* __restrict__ sums_back, unsigned int* __restrict__ step_out,
    int fail_ppt, int drop_ppt, int cap, int world)
{
    if (i >= world * cap) return;
    if ((i % cap) >= min(send_cnt[i / cap], cap)) return;
    const int sslot = send_slots[i];
    const int tag = sslot >= 0 ? child_tag[sslot] : rq_prev_tag[-1 - sslot];
    const int seq = sslot >= 0 ? child_seq[sslot] : rq_prev_seq[-1 - sslot];
    // lost-result injection (crashed worker): the child simply vanishes;
    // children_out stays up and the K4-WF timeout scan recovers it later
    const unsigned int hd = wf_mix((unsigned int)tag * 0x85EBCA6Bu
                                   ^ (unsigned int)seq * 0xC2B2AE35u);
    if ((int)(hd % 1000u) < drop_ppt) return;
    const unsigned int h = wf_mix((unsigned int)tag * 2654435761u
                                  ^ (unsigned int)seq * 40503u);
    if ((int)(h % 1000u) < fail_ppt) {
        atomicAdd(&children_fail[tag], 1);
    } else {
        atomicAdd(&children_done[tag], 1);
        // the step's output: wraparound sum of its succeeded children's
        // result words (addition mod 2^32 commutes: order cannot matter)
        if (OUT) atomicAdd(&step_out[tag], sums_back[i]);
    }
    atomicSub(&children_out[tag], 1);
}

__global__ __launch_bounds__(BLOCK) void wf_apply_kernel(
    const int* __restrict__ send_slots,       // [world*cap]
    const int* __restrict__ send_cnt,         // [world]
    const int* __restrict__ child_tag,        // [CB]
    const int* __restrict__ child_seq,        // [CB]
    const int* __restrict__ rq_prev_tag,      // [rq_cap]
    const int* __restrict__ rq_prev_seq,      // [rq_cap]
    int* __restrict__ children_done,          // [NR*64]
    int* __restrict__ children_fail,          // [NR*64]
    int* __restrict__ children_out,           // [NR*64]
    int fail_ppt, int drop_ppt, int cap, int world)
{
    wf_apply_one<false>(blockIdx.x * BLOCK + threadIdx.x, send_slots, send_cnt, child_tag,
                        child_seq, rq_prev_tag, rq_prev_seq, children_done, children_fail,
                        children_out, nullptr, nullptr, fail_ppt, drop_ppt, cap, world);
}

// wf_apply with step outputs (device conditions): sums_back[i] is the echo
// checksum of send entry i, step_out[tag] the output word of step tag
__global__ __launch_bounds__(BLOCK) void wf_apply_out_kernel(
    const int* __restrict__ send_slots, const int* __restrict__ send_cnt,
    const int* __restrict__ child_tag, const int* __restrict__ child_seq,
    const int* __restrict__ rq_prev_tag, const int* __restrict__ rq_prev_seq,
    int* __restrict__ children_done, int* __restrict__ children_fail,
    int* __restrict__ children_out,
    const unsigned int* __restrict__ sums_back,   // [world*cap]
    unsigned int* __restrict__ step_out,          // [NR*64]
    int fail_ppt, int drop_ppt, int cap, int world)
{
    wf_apply_one<true>(blockIdx.x * BLOCK + threadIdx.x, send_slots, send_cnt, child_tag,
                       child_seq, rq_prev_tag, rq_prev_seq, children_done, children_fail,
                       children_out, sums_back, step_out, fail_ppt, drop_ppt, cap, world);
}

// dead-letter application: entries dropped by the requeue ring (max-deliver
// exceeded / ring full) count as failed children so their steps can retry or
// fail instead of hanging forever
__global__ __launch_bounds__(BLOCK) void wf_apply_dead_kernel(
    const int* __restrict__ dead_src,         // [dcap] slot or -1-j flags
    const int* __restrict__ dead_count,       // [1]
    const int* __restrict__ child_tag,
    const int* __restrict__ rq_prev_tag,
    int* __restrict__ children_fail,
    int* __restrict__ children_out,
    int dcap)
{
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= min(*dead_count, dcap)) return;
    const int s = dead_src[i];
    const int tag = s >= 0 ? child_tag[s] : rq_prev_tag[-1 - s];
    atomicAdd(&children_fail[tag], 1);
    atomicSub(&children_out[tag], 1);
}

// K4-WF: stale-step timeout scan (reconciler.go:88-144 analog over the
// run/step table). A step DISPATCHED for > cutoff ticks with children still
// outstanding has lost them (worker crash / dropped result): the remainder
// is declared TIMEOUT — counted, converted to failed children — so the
// commit pass retries them with backoff instead of hanging forever.
// wf_write_off is that rule for one DISPATCHED step, shared with wf_settle: if
// the step's `out` children are due it clears children_out and calls
// `lost(out)`, where the caller books them as failed and counts them.
// `timeout` is called only for a step that has children out.
template <class Timeout, class Lost>
__device__ __forceinline__ void wf_write_off(size_t i, int out, int tick, const int* dispatch_tick,
                                             int* children_out, Timeout timeout, Lost lost) {
    if (out <= 0 || dispatch_tick[i] > tick - timeout()) return;
    children_out[i] = 0;
    lost(out);
}

__global__ __launch_bounds__(BLOCK) void wf_timeout_scan_kernel(
    const unsigned char* __restrict__ step_state,
    int* __restrict__ children_out,
    int* __restrict__ children_fail,
    const int* __restrict__ dispatch_tick,    // [NR*64] last expansion tick
    const int* __restrict__ tick_p, int cutoff,
    unsigned long long* __restrict__ timeout_count,
    int NRS)
{
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= NRS) return;
    if (step_state[i] != WFS_DISPATCHED) return;
    wf_write_off(i, children_out[i], *tick_p, dispatch_tick, children_out, [&] { return cutoff; },
                 [&](int lost) {
                     children_fail[i] += lost;
                     atomicAdd(timeout_count, (unsigned long long)lost);
                 });
}

// continuous re-admission (config #5 "hold 1M concurrent runs"): terminal
// runs in `filter_state` are reset from the creation template and re-enter
// the system. SUCCEEDED runs re-admit on device every tick; FAILED runs
// wait for the host DLQ drain (dlq_store.go analog) which re-admits them
// through the same kernel after recording the entries.
__global__ __launch_bounds__(BLOCK) void wf_readmit_kernel(
    unsigned char* __restrict__ run_active,
    unsigned char* __restrict__ run_state,
    const unsigned char* __restrict__ n_steps,
    unsigned char* __restrict__ step_state,
    int* __restrict__ step_attempts,
    int* __restrict__ children_todo,
    int* __restrict__ children_out,
    int* __restrict__ children_done,
    int* __restrict__ children_fail,
    int* __restrict__ children_emitted,
    int* __restrict__ next_ready,
    int* __restrict__ dispatch_tick,
    const int* __restrict__ todo_tmpl,        // [NR*64]
    const int* __restrict__ nready_tmpl,      // [NR*64]
    int filter_state,
    unsigned long long* __restrict__ admit_count,
    int NR)
{
    const int run = blockIdx.x * BLOCK + threadIdx.x;
    if (run >= NR) return;
    if (run_active[run] || run_state[run] != filter_state) return;
    const int ns = n_steps[run];
    const size_t base = (size_t)run * 64;
    for (int s = 0; s < ns; ++s) {
        const size_t i = base + s;
        step_state[i] = WFS_PENDING;
        step_attempts[i] = 0;
        children_todo[i] = todo_tmpl[i];
        children_out[i] = 0;
        children_done[i] = 0;
        children_fail[i] = 0;
        children_emitted[i] = 0;
        next_ready[i] = nready_tmpl[i];
        dispatch_tick[i] = 0;
    }
    run_state[run] = 0;
    run_active[run] = 1;
    atomicAdd(admit_count, 1ull);
}

// step commit: aggregate children (engine.go:1623-1645) + retry/backoff
// (computeBackoff :1573-1595, attempts capped by max_retries).
// wf_commit_step is the rule for one DISPATCHED step, shared by wf_commit and
// wf_settle. `out` and `fail` are its children_out and children_fail (after a
// write-off, if any). It ends in `done(next state, children sent to retry)`;
// on a retry it has advanced step_attempts, children_todo and next_ready, and
// the caller owes children_fail = 0 and its retry counter. `load_policy()` is
// called on the failed-children branch only and gives .max_retries and
// .backoff(attempt). `done` is a callable, not a return value, so that each
// branch keeps the direct stores it had in wf_commit.
template <class LoadPolicy, class Done>
__device__ __forceinline__ void wf_commit_step(
    size_t i, int out, int fail, int tick, int* step_attempts, int* children_todo,
    const int* max_parallel, int* next_ready, LoadPolicy load_policy, Done done) {
    if (out != 0) {
        // window slide: with children still in flight, re-open emission as
        // soon as there is BOTH work left and room (max_parallel window, or
        // freed child-arena space for the unlimited case); max_parallel is
        // read only with work left
        const bool room = children_todo[i] > 0
                          && (max_parallel[i] == 0 || out < max_parallel[i]);
        return done(room ? WFS_PENDING : WFS_DISPATCHED, 0);
    }
    if (fail > 0) {
        const auto policy = load_policy();
        const int att = step_attempts[i];
        if (att >= policy.max_retries) return done(WFS_FAILED, 0);
        step_attempts[i] = att + 1;
        children_todo[i] += fail;                   // only failed children re-run
        next_ready[i] = tick + policy.backoff(att + 1);
        return done(WFS_PENDING, fail);
    }
    // partial emission resumes, or the step is done
    done(children_todo[i] > 0 ? WFS_PENDING : WFS_SUCCEEDED, 0);
}

// wf_commit's policy: backoff min(2^attempt, 16); the shift is capped at 4 so
// an attempt count past the width of an int cannot wrap the delay
struct wf_stock_policy {
    int max_retries;
    __device__ __forceinline__ int backoff(int attempt) const { return 1 << min(attempt, 4); }
};

__global__ __launch_bounds__(BLOCK) void wf_commit_kernel(
    unsigned char* __restrict__ step_state,   // [NR*64]
    int* __restrict__ step_attempts,          // [NR*64]
    int* __restrict__ children_todo,
    int* __restrict__ children_out,
    int* __restrict__ children_done,          // kept: successes accumulate
    int* __restrict__ children_fail,
    const int* __restrict__ max_parallel,
    int* __restrict__ next_ready,
    const int* __restrict__ tick_p, int max_retries,
    unsigned long long* __restrict__ retry_count,  // cumulative children retried
    int NRS)
{
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= NRS) return;
    if (step_state[i] != WFS_DISPATCHED) return;
    const int out = children_out[i];
    const int fail = out != 0 ? 0 : children_fail[i];   // read only where the rule uses it
    wf_commit_step(
        i, out, fail, *tick_p, step_attempts, children_todo, max_parallel, next_ready,
        [&] { return wf_stock_policy{max_retries}; },
        [&](int next, int retried) {
            if (next != WFS_DISPATCHED) step_state[i] = (unsigned char)next;
            if (retried > 0) {
                children_fail[i] = 0;
                atomicAdd(retry_count, (unsigned long long)retried);
            }
        });
}

// run status roll-up (updateRunStatus :1647-1699): all steps SUCCEEDED or
// SKIPPED -> run SUCCEEDED; any FAILED step -> run FAILED (retries already
// exhausted at step level). counts[0] += succeeded, counts[1] += failed.
__global__ __launch_bounds__(BLOCK) void wf_status_kernel(
    const unsigned char* __restrict__ step_state,
    const unsigned char* __restrict__ n_steps,
    unsigned char* __restrict__ run_active,
    unsigned char* __restrict__ run_state,    // [NR] WFS_* of the run
    unsigned long long* __restrict__ counts,  // [2]
    int NR)
{
    const int run = blockIdx.x * BLOCK + threadIdx.x;
    if (run >= NR || !run_active[run]) return;
    const int ns = n_steps[run];
    const unsigned char* st = &step_state[(size_t)run * 64];
    bool all_ok = true, any_fail = false;
    for (int s = 0; s < ns; ++s) {
        const unsigned char v = st[s];
        any_fail |= (v == WFS_FAILED);
        all_ok &= (v == WFS_SUCCEEDED || v == WFS_SKIPPED);
    }
    if (any_fail) {
        run_active[run] = 0;
        run_state[run] = WFS_FAILED;
        atomicAdd(&counts[1], 1ull);
    } else if (all_ok) {
        run_active[run] = 0;
        run_state[run] = WFS_SUCCEEDED;
        atomicAdd(&counts[0], 1ull);
    }
}

// host-driven approval grants (the admin hop): verdict 1 -> SUCCEEDED,
// 0 -> FAILED (rejection fails the step, which fails the run)
__global__ __launch_bounds__(BLOCK) void wf_grant_kernel(
    const int* __restrict__ grant_runs,
    const int* __restrict__ grant_steps,
    const unsigned char* __restrict__ verdicts,
    int n,
    unsigned char* __restrict__ step_state)
{
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const size_t rs = (size_t)grant_runs[i] * 64 + grant_steps[i];
    if (step_state[rs] == WFS_WAITING)
        step_state[rs] = verdicts[i] ? WFS_SUCCEEDED : WFS_FAILED;
}

// ---------------------------------------------------------------------------
// K3-WF run lifecycle: admit / cancel / retire between ticks
// ---------------------------------------------------------------------------
// Dynamic mode of the workflow engine: a run slot is FREE, LIVE (admitted,
// running or terminal-but-unreported) or DRAINING (terminal and reported,
// children may still be parked in the requeue ring). A host handle is
// (slot, generation); run_gen[slot] increments at each admission, so a stale
// handle can never cancel the slot's next occupant (CancelRun analog,
// workflow/engine.go:349-451). All three kernels run between ticks, outside
// the captured graph, and read the device tick counter.
//
// Invariant: a slot is never handed to a new run while a child of its
// previous occupant can still be applied to it. wf_retire frees a DRAINING
// row only when every step has no child out, or its last expansion is older
// than the timeout cutoff, which exceeds the longest requeue-ring lifetime.
//
// A cancelled step is WFS_CANCELLED: sweep, expand, timeout scan, commit and
// status only ever act on the states 0..5 they name, so they leave it alone.
#define WFS_CANCELLED 6
#define WFL_FREE 0
#define WFL_LIVE 1
#define WFL_DRAINING 2

// admission pass 1: free-slot bitmask per wave (4 per 256-slot block) and
// the free count per block. The masks are a snapshot: the admit pass reads
// them, never run_life, so its waves cannot race on the table they fill.
__global__ __launch_bounds__(BLOCK) void wf_admit_count_kernel(
    const unsigned char* __restrict__ run_life,   // [NR]
    unsigned long long* __restrict__ free_mask,   // [nblk*4]
    int* __restrict__ blk_scan,                   // [nblk+1] counts, scanned next
    int NR)
{
    const int run = blockIdx.x * BLOCK + threadIdx.x;
    const int w = threadIdx.x / WAVE;
    const unsigned long long m =
        __ballot(run < NR && run_life[run] == WFL_FREE);
    if (threadIdx.x % WAVE == 0)
        free_mask[(size_t)blockIdx.x * (BLOCK / WAVE) + w] = m;
    const int free = block_sum((int)__popcll(m));
    if (threadIdx.x == 0) blk_scan[blockIdx.x] = free;
}

// admission pass 2: in-place exclusive scan of the block counts by one
// workgroup (4096 entries at one million slots); blk_scan[nblk] = total free
__global__ __launch_bounds__(BLOCK) void wf_admit_scan_kernel(
    int* __restrict__ blk_scan, int nblk)
{
    __shared__ int part[BLOCK];
    const int chunk = (nblk + BLOCK - 1) / BLOCK;
    const int lo = min((int)threadIdx.x * chunk, nblk);
    const int hi = min(lo + chunk, nblk);
    int sum = 0;
    for (int j = lo; j < hi; ++j) sum += blk_scan[j];
    part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int t = 0; t < BLOCK; ++t) { const int v = part[t]; part[t] = run; run += v; }
        blk_scan[nblk] = run;
    }
    __syncthreads();
    int run = part[threadIdx.x];
    for (int j = lo; j < hi; ++j) { const int v = blk_scan[j]; blk_scan[j] = run; run += v; }
}

// the i-th lowest FREE slot of the snapshot (i below the free total), or -1:
// binary search over the scanned block counts, then popcounts over the
// block's four masks. Wave-uniform.
__device__ __forceinline__ int wf_admit_place(
    int i, int lane, const unsigned long long* __restrict__ free_mask,
    const int* __restrict__ blk_scan, int nblk, int NR)
{
    // largest block b with blk_scan[b] <= i (empty blocks share a prefix)
    int lo = 0, hi = nblk - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (blk_scan[mid] <= i) lo = mid; else hi = mid - 1;
    }
    int k = i - blk_scan[lo];
    int g = 0;
    unsigned long long m = free_mask[(size_t)lo * 4];
    while (g < 3 && k >= __popcll(m)) {
        k -= __popcll(m);
        ++g;
        m = free_mask[(size_t)lo * 4 + g];
    }
    // the k-th set bit of m: the one lane whose bit is set with k below it
    const unsigned long long pick = __ballot(
        ((m >> lane) & 1ull) && __popcll(m & ((1ull << lane) - 1ull)) == k);
    const int slot = lo * BLOCK + g * WAVE + (__ffsll((long long)pick) - 1);
    return (pick == 0ull || slot >= NR) ? -1 : slot;   // -1 cannot happen: masks and scan agree
}

// the row of an admitted run, by its wave: lane s writes step s of `slot`
// from template `tid` (steps at and past the template's n_steps are zero),
// lane 0 the run columns and the handle. `state` is the lane's step state:
// the one entry that differs between a fresh admission and one with kept steps.
__device__ __forceinline__ void wf_admit_row(
    int i, int lane, int slot, int tid, int ns, unsigned char state,
    const long long* __restrict__ req_cond,
    const int* __restrict__ req_fanout,
    const long long* __restrict__ tmpl_deps,
    const unsigned char* __restrict__ tmpl_kind,
    const int* __restrict__ tmpl_todo,
    const int* __restrict__ tmpl_maxp,
    const int* __restrict__ tmpl_delay,
    unsigned char* __restrict__ step_state,
    int* __restrict__ step_attempts,
    long long* __restrict__ deps_mask,
    unsigned char* __restrict__ step_kind,
    int* __restrict__ children_todo,
    int* __restrict__ max_parallel,
    int* __restrict__ children_out,
    int* __restrict__ children_done,
    int* __restrict__ children_fail,
    int* __restrict__ children_emitted,
    int* __restrict__ next_ready,
    int* __restrict__ dispatch_tick,
    unsigned char* __restrict__ n_steps,
    long long* __restrict__ cond_bits,
    unsigned char* __restrict__ run_state,
    unsigned char* __restrict__ run_active,
    unsigned char* __restrict__ run_life,
    int* __restrict__ run_gen,
    const int* __restrict__ tick_p,
    int* __restrict__ out_slot,
    int* __restrict__ out_gen)
{
    const int tick1 = *tick_p + 1;                // the run's first tick
    const bool in = lane < ns;
    const size_t ti = (size_t)tid * 64 + lane;
    const size_t ri = (size_t)slot * 64 + lane;
    const int kind = in ? (int)tmpl_kind[ti] : 0;
    const int fan = req_fanout[i];
    step_state[ri] = state;
    step_attempts[ri] = 0;
    deps_mask[ri] = in ? tmpl_deps[ti] : 0ll;
    step_kind[ri] = (unsigned char)kind;
    children_todo[ri] = !in ? 0 : (kind == WFK_FOR_EACH && fan > 0) ? fan : tmpl_todo[ti];
    max_parallel[ri] = in ? tmpl_maxp[ti] : 0;
    children_out[ri] = 0;
    children_done[ri] = 0;
    children_fail[ri] = 0;
    children_emitted[ri] = 0;
    next_ready[ri] = in ? tick1 + tmpl_delay[ti] : 0;
    dispatch_tick[ri] = in ? tick1 : 0;
    if (lane == 0) {
        n_steps[slot] = (unsigned char)ns;
        cond_bits[slot] = req_cond[i];
        run_state[slot] = 0;
        run_active[slot] = 1;
        run_life[slot] = WFL_LIVE;
        const int gen = run_gen[slot] + 1;
        run_gen[slot] = gen;
        out_slot[i] = slot;
        out_gen[i] = gen;
    }
}

#define WF_ADMIT_PARAMS \
    const int* __restrict__ req_tmpl,             /* [n] template id */ \
    const long long* __restrict__ req_cond,       /* [n] condition bits */ \
    const int* __restrict__ req_fanout,           /* [n] FOR_EACH override (0 = none) */ \
    int n, \
    const long long* __restrict__ tmpl_deps,      /* [TC*64] */ \
    const unsigned char* __restrict__ tmpl_kind,  /* [TC*64] */ \
    const int* __restrict__ tmpl_todo,            /* [TC*64] */ \
    const int* __restrict__ tmpl_maxp,            /* [TC*64] */ \
    const int* __restrict__ tmpl_delay,           /* [TC*64] */ \
    const unsigned char* __restrict__ tmpl_nsteps,/* [TC] */ \
    int TC, \
    const unsigned long long* __restrict__ free_mask, \
    const int* __restrict__ blk_scan, int nblk, \
    unsigned char* __restrict__ step_state, \
    int* __restrict__ step_attempts, \
    long long* __restrict__ deps_mask, \
    unsigned char* __restrict__ step_kind, \
    int* __restrict__ children_todo, \
    int* __restrict__ max_parallel, \
    int* __restrict__ children_out, \
    int* __restrict__ children_done, \
    int* __restrict__ children_fail, \
    int* __restrict__ children_emitted, \
    int* __restrict__ next_ready, \
    int* __restrict__ dispatch_tick, \
    unsigned char* __restrict__ n_steps, \
    long long* __restrict__ cond_bits, \
    unsigned char* __restrict__ run_state, \
    unsigned char* __restrict__ run_active, \
    unsigned char* __restrict__ run_life, \
    int* __restrict__ run_gen, \
    const int* __restrict__ tick_p, \
    int* __restrict__ out_slot,                   /* [n] */ \
    int* __restrict__ out_gen,                    /* [n] */ \
    unsigned long long* __restrict__ admit_count, \
    int NR
#define WF_ADMIT_ROW_ARGS \
    req_cond, req_fanout, tmpl_deps, tmpl_kind, tmpl_todo, tmpl_maxp, tmpl_delay, \
    step_state, step_attempts, deps_mask, step_kind, children_todo, max_parallel, \
    children_out, children_done, children_fail, children_emitted, next_ready, \
    dispatch_tick, n_steps, cond_bits, run_state, run_active, run_life, run_gen, \
    tick_p, out_slot, out_gen

// admission pass 3: one wave per request. Request i takes the i-th lowest
// FREE slot, a pure function of the tables and the request order. Its 64
// lanes write the 64-step row, one lane per step, so every table write is
// one coalesced 64-lane store.
__global__ __launch_bounds__(BLOCK) void wf_admit_kernel(WF_ADMIT_PARAMS)
{
    const int i = (blockIdx.x * BLOCK + threadIdx.x) / WAVE;
    const int lane = threadIdx.x % WAVE;
    if (i >= n) return;                           // wave-uniform
    const int total = blk_scan[nblk];
    if (i == 0 && lane == 0)
        atomicAdd(admit_count, (unsigned long long)min(n, total));
    const int slot = i < total ? wf_admit_place(i, lane, free_mask, blk_scan, nblk, NR) : -1;
    if (slot < 0) {                               // table full
        if (lane == 0) { out_slot[i] = -1; out_gen[i] = 0; }
        return;
    }
    const int tid = req_tmpl[i];
    const bool known = tid >= 0 && tid < TC;      // host rejects the rest
    const int ns = known ? (int)tmpl_nsteps[tid] : 0;
    wf_admit_row(i, lane, slot, known ? tid : 0, ns, WFS_PENDING, WF_ADMIT_ROW_ARGS);
}

// admission with kept steps (rerun from a step): wf_admit_kernel's placement
// and row, with the steps named by req_keep already done: SKIPPED where
// req_skip names them too, SUCCEEDED otherwise. The kept set has to lie
// inside the template's steps and be closed under its dependencies; a request
// that is not gets -2 and writes nothing else. That is decided first, from
// the request and the template alone, so -2 wins over a full table, and the
// i-th free slot of such a request i stays FREE: valid requests land where
// their index puts them, whatever their neighbours are.
__global__ __launch_bounds__(BLOCK) void wf_admit_keep_kernel(
    WF_ADMIT_PARAMS,
    const long long* __restrict__ req_keep,       // [n] bit s: step s is done
    const long long* __restrict__ req_skip)       // [n] bit s: ... as SKIPPED
{
    const int i = (blockIdx.x * BLOCK + threadIdx.x) / WAVE;
    const int lane = threadIdx.x % WAVE;
    if (i >= n) return;                           // wave-uniform
    const int req = req_tmpl[i];
    const bool known = req >= 0 && req < TC;      // host rejects the rest
    const int tid = known ? req : 0;
    const int ns = known ? (int)tmpl_nsteps[tid] : 0;
    const unsigned long long keep = (unsigned long long)req_keep[i];
    const unsigned long long skip = (unsigned long long)req_skip[i] & keep;
    const bool kept = (keep >> lane) & 1ull;
    // a 64-step template has no bit past its steps: never shift by 64
    const bool past = ns < 64 && (keep >> ns) != 0ull;
    const bool open = kept && lane < ns
        && ((unsigned long long)tmpl_deps[(size_t)tid * 64 + lane] & ~keep) != 0ull;
    if (past || __ballot(open) != 0ull) {         // wave-uniform
        if (lane == 0) { out_slot[i] = -2; out_gen[i] = 0; }
        return;
    }
    const int total = blk_scan[nblk];
    const int slot = i < total ? wf_admit_place(i, lane, free_mask, blk_scan, nblk, NR) : -1;
    if (slot < 0) {                               // table full
        if (lane == 0) { out_slot[i] = -1; out_gen[i] = 0; }
        return;
    }
    if (lane == 0) atomicAdd(admit_count, 1ull);  // a count, not a placement
    const unsigned char state = !kept ? WFS_PENDING
        : ((skip >> lane) & 1ull) ? WFS_SKIPPED : WFS_SUCCEEDED;
    wf_admit_row(i, lane, slot, tid, ns, state, WF_ADMIT_ROW_ARGS);
}

// cancellation: one wave per request (distinct slots), one lane per step.
// Effective only on a LIVE, still-active run of the named generation; the
// child counters are left alone, so children in flight still apply into the
// quarantined row and the retire pass can tell when it is quiet.
__global__ __launch_bounds__(BLOCK) void wf_cancel_kernel(
    const int* __restrict__ req_slot,             // [n]
    const int* __restrict__ req_gen,              // [n]
    int n,
    const unsigned char* __restrict__ run_life,
    const int* __restrict__ run_gen,
    unsigned char* __restrict__ run_active,
    unsigned char* __restrict__ run_state,
    const unsigned char* __restrict__ n_steps,
    unsigned char* __restrict__ step_state,
    unsigned long long* __restrict__ cancel_count,
    unsigned char* __restrict__ out_ok,           // [n]
    int NR)
{
    const int i = (blockIdx.x * BLOCK + threadIdx.x) / WAVE;
    const int lane = threadIdx.x % WAVE;
    if (i >= n) return;                           // wave-uniform
    const int slot = req_slot[i];
    int ok = 0;
    if (lane == 0 && slot >= 0 && slot < NR)
        ok = run_life[slot] == WFL_LIVE && run_gen[slot] == req_gen[i]
             && run_active[slot] == 1;
    ok = __shfl(ok, 0, WAVE);
    if (!ok) {
        if (lane == 0) out_ok[i] = 0;
        return;
    }
    if (lane < (int)n_steps[slot]) {
        const size_t ri = (size_t)slot * 64 + lane;
        const unsigned char s = step_state[ri];
        if (s == WFS_PENDING || s == WFS_DISPATCHED || s == WFS_WAITING)
            step_state[ri] = WFS_CANCELLED;
    }
    if (lane == 0) {
        run_active[slot] = 0;
        run_state[slot] = WFS_CANCELLED;
        out_ok[i] = 1;
        atomicAdd(cancel_count, 1ull);
    }
}

// retirement: one thread per run for the one-byte life filter; terminal LIVE
// runs are appended to the done list (wave-aggregated, order undefined) and
// become DRAINING. Each DRAINING run, including one set just now, gets a
// wave-cooperative row check: all 64 lanes read the chosen run's row. A
// call that finds few terminal runs reads the life bytes, not the rows.
__global__ __launch_bounds__(BLOCK) void wf_retire_kernel(
    unsigned char* __restrict__ run_life,         // [NR]
    const unsigned char* __restrict__ run_active,
    const unsigned char* __restrict__ run_state,
    const int* __restrict__ run_gen,
    const unsigned char* __restrict__ n_steps,
    const int* __restrict__ children_out,         // [NR*64]
    const int* __restrict__ dispatch_tick,        // [NR*64]
    const int* __restrict__ tick_p, int cutoff,
    int* __restrict__ done_slot,                  // [cap]
    int* __restrict__ done_gen,
    int* __restrict__ done_state,
    int* __restrict__ done_count,                 // [1]
    int NR, int cap)
{
    const int run = blockIdx.x * BLOCK + threadIdx.x;
    const int lane = threadIdx.x % WAVE;
    const int life = run < NR ? (int)run_life[run] : WFL_FREE;
    const bool report = life == WFL_LIVE && run_active[run] == 0;
    const int pos = wave_append_slot(report, done_count, lane);
    if (pos >= 0 && pos < cap) {
        done_slot[pos] = run;
        done_gen[pos] = run_gen[run];
        done_state[pos] = run_state[run];
    }
    const bool draining = report || life == WFL_DRAINING;
    const int stale = *tick_p - cutoff;
    unsigned long long todo = __ballot(draining);
    bool quiet = false;
    while (todo != 0ull) {                        // wave-uniform loop
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1ull;
        const int r = __shfl(run, src, WAVE);
        const size_t ri = (size_t)r * 64 + lane;
        const bool blocking = lane < (int)n_steps[r] && children_out[ri] > 0
                              && dispatch_tick[ri] > stale;
        const bool q = !__any(blocking);
        if (lane == src) quiet = q;
    }
    if (draining) {
        const int next = quiet ? WFL_FREE : WFL_DRAINING;
        if (next != life) run_life[run] = (unsigned char)next;
    }
}

// step-transition journal: an observer of the tables above. It compares
// every step state of the LIVE and DRAINING rows with the state it last
// reported (ev_shadow_state) and appends one 16-byte record per difference:
//   word0 slot | word1 gen | word2 step | from<<8 | to<<16 | word3 2*tick+phase
// A row whose generation differs from ev_shadow_gen was admitted since its
// shadow was written: its shadow counts as all PENDING, the image wf_admit
// writes, and the admission itself is no event. FREE rows cost their life
// byte only.
//
// Row-scan layout (see the helpers above K3), the shadow read like the states.
// A wave with no difference and no generation change leaves after the loads.
// Otherwise it reserves list space with one atomic for the whole wave
// (per-lane counts, wave prefix sum); a record at a position >= cap is not
// written and its shadow byte does not advance, so the next pass finds the
// change again: a full list delays and coalesces events, it loses none.
//
// ev_count: a wave adds to it only if it read it below cap, and adds at most
// 1024 (16 rows x 64 steps). Every wave of a pass can do that once, so
//   ev_count <= max(cap - 1, value at entry) + 64 * NR
// however many passes run before the host drains it. The host binding
// rejects tables for which that could wrap.
__global__ __launch_bounds__(BLOCK) void wf_journal_kernel(
    const unsigned char* __restrict__ step_state,   // [NR*64]
    const unsigned char* __restrict__ run_life,     // [NR]
    const int* __restrict__ run_gen,                // [NR]
    const int* __restrict__ tick_p, int phase,
    unsigned char* __restrict__ ev_shadow_state,    // [NR*64]
    int* __restrict__ ev_shadow_gen,                // [NR]
    int* __restrict__ ev_rec,                       // [cap*4]
    int* __restrict__ ev_count,                     // [1]
    int NR, int cap)
{
    const auto [r, q, off] = wf_row_coords();
    const int lane = threadIdx.x % WAVE;
    const bool live = r < NR && run_life[r] != WFL_FREE;
    int gen = 0;
    bool regen = false;
    wf_bytes16 st = {}, sh = {};                    // WFS_PENDING == 0
    if (live) {
        gen = run_gen[r];
        regen = gen != ev_shadow_gen[r];
        st = load16(step_state + off);
        if (!regen) sh = load16(ev_shadow_state + off);
    }
    const unsigned diff = differ16(st, sh);         // bit j: step 16q+j differs
    const int n = __popc(diff);
    if (!__any(n > 0 || regen)) return;             // wave-uniform early exit

    const int incl = wave_prefix_sum(n, lane);
    const int total = __shfl(incl, WAVE - 1, WAVE);
    int base = 0;
    if (lane == 0 && total > 0) {
        const int seen = __hip_atomic_load(ev_count, __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT);
        base = seen >= cap ? cap : atomicAdd(ev_count, total);
    }
    base = __shfl(base, 0, WAVE);
    int pos = base + incl - n;
    const int stamp = 2 * *tick_p + phase;
    wf_bytes16 now = sh;                            // the shadow after this pass
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        if ((diff >> j) & 1u) {
            if (pos < cap) {
                const unsigned from = byte16(sh, j), to = byte16(st, j);
                *reinterpret_cast<int4*>(ev_rec + (size_t)pos * 4) = make_int4(
                    r, gen, (int)((unsigned)(q * 16 + j) | from << 8 | to << 16), stamp);
                set_byte(now, j, to);
            }
            ++pos;
        }
    }
    // a re-admitted row's stale shadow is replaced whole; otherwise the
    // shadow is written only where an event advanced it
    store16_if_changed(ev_shadow_state + off, now, sh, regen);
    if (regen && q == 0) ev_shadow_gen[r] = gen;
}

// ---------------------------------------------------------------------------
// K3-WF per-step retry / backoff / timeout policy: wf_settle
// ---------------------------------------------------------------------------
// With a per-step policy the tick launches wf_settle in place of the pair
// wf_timeout_scan + wf_commit. Both of those act on index i only, so running
// them back to back per step is the same computation, and it is the same
// code: wf_write_off, then wf_commit_step. The policy is held per template
// (templates are append-only), and run_tmpl[r] names the template of the
// row's occupant:
//   tmpl_policy[(t*64+s)*4 ..] = (max_retries, backoff_ticks, cap_ticks,
//                                 multiplier_q8), one 16-byte record per step
//   tmpl_timeout[t*64+s]       = ticks after which outstanding children are
//                                 written off (resolved: never 0, never below
//                                 the pipeline's cutoff)
// The host validates the records (wf_pipeline.py); the kernel trusts their
// ranges and checks only that the template id is inside the table. A row
// whose id is not is left alone.
//
// What still differs from the pair:
//   - the constants: launch arguments and wf_stock_policy there, the
//     template's timeout and policy record (wf_step_policy) here;
//   - FREE rows are skipped. With a step timeout longer than the pipeline
//     cutoff wf_retire can free a row that still holds a DISPATCHED step with
//     children counted outstanding; its bytes belong to nobody and the next
//     admission overwrites them;
//   - the counters get one add per block, not per step, and children_fail
//     one store per step, after write-off and retry, not one in each.
//
// backoff(k), integers only (16.16 fixed point, multiplier in 8.8); the
// oracle (reference.wf_backoff_ref) uses the same arithmetic:
//   limit = (cap_ticks > 0 ? cap_ticks : 1<<20) << 16
//   d = min(backoff_ticks << 16, limit)
//   min(k-1, 63) times, stopping once d == limit: d = min((d*mult_q8) >> 8, limit)
//   backoff = (d + 65535) >> 16
// d <= 2^36 and mult_q8 < 2^16 for validated records, so d*mult_q8 < 2^52.
__device__ __forceinline__ int wf_backoff_ticks(int k, int backoff_ticks, int cap_ticks,
                                                int mult_q8)
{
    const unsigned long long limit =
        (unsigned long long)(cap_ticks > 0 ? cap_ticks : (1 << 20)) << 16;
    unsigned long long d = min((unsigned long long)(unsigned)backoff_ticks << 16, limit);
    const int n = min(k - 1, 63);
#pragma unroll 1
    for (int i = 0; i < n && d != limit; ++i)
        d = min((d * (unsigned long long)(unsigned)mult_q8) >> 8, limit);
    return (int)((d + 65535ull) >> 16);
}

// one record of tmpl_policy: max_retries, backoff_ticks, cap_ticks, multiplier_q8
struct wf_step_policy {
    int max_retries, backoff_ticks, cap_ticks, mult_q8;
    __device__ __forceinline__ int backoff(int attempt) const {
        return wf_backoff_ticks(attempt, backoff_ticks, cap_ticks, mult_q8);
    }
};

// Row-scan layout (see the helpers above K3). A FREE row costs its life byte.
// A wave with no DISPATCHED byte does nothing more after the loads and writes
// nothing. Only a lane that holds a DISPATCHED byte reads run_tmpl and the
// counter columns of those steps, and only a step with failed children and
// none outstanding reads its policy record.
__global__ __launch_bounds__(BLOCK) void wf_settle_kernel(
    unsigned char* __restrict__ step_state,         // [NR*64]
    int* __restrict__ step_attempts,                // [NR*64]
    int* __restrict__ children_todo,
    int* __restrict__ children_out,
    int* __restrict__ children_fail,
    const int* __restrict__ max_parallel,
    int* __restrict__ next_ready,
    const int* __restrict__ dispatch_tick,          // [NR*64]
    const unsigned char* __restrict__ run_life,     // [NR]
    const int* __restrict__ run_tmpl,               // [NR]
    const int4* __restrict__ tmpl_policy,           // [TC*64]
    const int* __restrict__ tmpl_timeout,           // [TC*64]
    const int* __restrict__ tick_p,
    unsigned long long* __restrict__ timeout_count,
    unsigned long long* __restrict__ retry_count,
    int NR, int TC)
{
    const auto [r, q, off] = wf_row_coords();
    const bool live = r < NR && run_life[r] != WFL_FREE;
    wf_bytes16 st = {};                             // WFS_PENDING == 0
    if (live) st = load16(step_state + off);
    unsigned disp = match16(st, WFS_DISPATCHED);    // bit j: step 16q+j is DISPATCHED

    unsigned long long sums[2] = {0ull, 0ull};      // children lost, children retried
    if (__any(disp != 0u)) {                        // wave-uniform
        if (disp != 0u) {
            const int tmpl = run_tmpl[r];
            if (tmpl < 0 || tmpl >= TC) disp = 0u;  // no such template: leave the row
            const size_t pol = (size_t)tmpl * 64 + (size_t)q * 16;
            const int tick = *tick_p;
            wf_bytes16 now = st;
#pragma unroll 1
            for (unsigned f = disp; f != 0u; f &= f - 1u) {
                const int j = __ffs((int)f) - 1;
                const size_t i = off + j;
                int out = children_out[i];
                int fail = children_fail[i];
                const int fail0 = fail;
                // 1. timeout: the remainder is lost and counts as failed
                wf_write_off(i, out, tick, dispatch_tick, children_out,
                             [&] { return tmpl_timeout[pol + j]; },
                             [&](int lost) { fail += lost; sums[0] += lost; out = 0; });
                // 2. commit
                int next = WFS_DISPATCHED;
                wf_commit_step(
                    i, out, fail, tick, step_attempts, children_todo, max_parallel, next_ready,
                    [&] { const int4 p = tmpl_policy[pol + j];
                          return wf_step_policy{p.x, p.y, p.z, p.w}; },
                    [&](int to, int retried) { next = to; sums[1] += retried; fail -= retried; });
                if (fail != fail0) children_fail[i] = fail;
                set_byte(now, j, (unsigned)next);
            }
            store16_if_changed(step_state + off, now, st);
        }
        sums[0] = wave_sum(sums[0]);
        sums[1] = wave_sum(sums[1]);
    }
    block_sum(sums);
    if (threadIdx.x == 0) {
        if (sums[0]) atomicAdd(timeout_count, sums[0]);
        if (sums[1]) atomicAdd(retry_count, sums[1]);
    }
}

// ---------------------------------------------------------------------------
// K3-WF conditions decided on the device: wf_cond_eval / wf_child_payload
// ---------------------------------------------------------------------------
// A step may carry a predicate over the run's input words and the output
// words of steps it (transitively) depends on. Predicates are held per
// template, one 16-byte record (code, a, b, imm) per step:
//   code bits 0..3   op: 0 none, 1 EQ, 2 NE, 3 LT, 4 LE, 5 GT, 6 GE,
//                    7 TRUTHY (lhs != 0, rhs ignored)
//        bit  4      negate the result
//        bits 8..9   lhs kind: 1 INPUT, 2 OUT
//        bits 12..13 rhs kind: 0 IMM, 1 INPUT, 2 OUT
//   a, b             lhs / rhs index (input word, or step), imm the immediate
// All comparisons are signed 32-bit. tmpl_cond_mask[t] bit s = step s of
// template t has a predicate. The host validates the records; the kernel
// still reads an operand whose index is outside its row as 0.
#define WFC_EQ 1
#define WFC_NE 2
#define WFC_LT 3
#define WFC_LE 4
#define WFC_GT 5
#define WFC_GE 6
#define WFC_TRUTHY 7

__device__ __forceinline__ int wf_cond_operand(int kind, int idx, int imm,
                                               const int* __restrict__ in_row, int IW,
                                               const int* __restrict__ out_row)
{
    if (kind == 1) return (unsigned)idx < (unsigned)IW ? in_row[idx] : 0;
    if (kind == 2) return (unsigned)idx < 64u ? out_row[idx] : 0;
    return imm;
}

__device__ __forceinline__ bool wf_cond_value(const int4 rec,
                                              const int* __restrict__ in_row, int IW,
                                              const int* __restrict__ out_row)
{
    const int code = rec.x;
    const int lk = (code >> 8) & 3;
    const int lhs = wf_cond_operand(lk == 0 ? 3 : lk, rec.y, 0, in_row, IW, out_row);
    const int rhs = wf_cond_operand((code >> 12) & 3, rec.z, rec.w, in_row, IW, out_row);
    bool v = false;
    switch (code & 15) {
    case WFC_EQ: v = lhs == rhs; break;
    case WFC_NE: v = lhs != rhs; break;
    case WFC_LT: v = lhs < rhs; break;
    case WFC_LE: v = lhs <= rhs; break;
    case WFC_GT: v = lhs > rhs; break;
    case WFC_GE: v = lhs >= rhs; break;
    case WFC_TRUTHY: v = lhs != 0; break;
    }
    return v != (((code >> 4) & 1) != 0);
}

// wf_cond_eval runs directly before wf_sweep. Row-scan layout (see the helpers
// above K3). A row is looked at only if it is LIVE, run_active is set and
// run_tmpl is inside the table; the four lanes OR their shares of `satisfied`
// (SUCCEEDED or SKIPPED, as the sweep). A wave in which no row has a PENDING
// step with a predicate does nothing more and writes nothing. A PENDING
// predicate step whose deps are satisfied is evaluated:
//   CONDITION  its bit in cond_bits[run] is set or cleared and step_out is
//              1 or 0; the sweep of this tick commits it, unchanged
//   guard      true: the step stays PENDING; false: it becomes SKIPPED
// A step skipped here satisfies its dependents in the sweep of this same
// tick, so the pass repeats (wave-uniform) until no guard turned false:
// otherwise the sweep would dispatch a dependent whose own guard was never
// looked at. Each step is evaluated at most once per launch. next_ready is
// not consulted: operands are final and inputs constant, so a step that
// returns to PENDING (retry, for_each window) evaluates the same again.
// cond_bits[run] is written once per row by lane q == 0; cond_counts (true,
// false) gets at most one atomic add per counter and block.
__global__ __launch_bounds__(BLOCK) void wf_cond_eval_kernel(
    unsigned char* __restrict__ step_state,         // [NR*64]
    const long long* __restrict__ deps_mask,        // [NR*64]
    const unsigned char* __restrict__ step_kind,    // [NR*64]
    const unsigned char* __restrict__ run_life,     // [NR]
    const unsigned char* __restrict__ run_active,   // [NR]
    const int* __restrict__ run_tmpl,               // [NR]
    const int4* __restrict__ tmpl_cond,             // [TC*64]
    const unsigned long long* __restrict__ tmpl_cond_mask, // [TC]
    const int* __restrict__ run_input,              // [NR*IW]
    int* __restrict__ step_out,                     // [NR*64]
    unsigned long long* __restrict__ cond_bits,     // [NR]
    unsigned long long* __restrict__ cond_counts,   // [2] true, false
    int NR, int TC, int IW)
{
    const auto [r, q, off] = wf_row_coords();
    bool look = r < NR && run_life[r] == WFL_LIVE && run_active[r] != 0;
    int tmpl = 0;
    if (look) {
        tmpl = run_tmpl[r];
        look = tmpl >= 0 && tmpl < TC;
    }
    wf_bytes16 st = {};
    unsigned long long cmask = 0ull;
    if (look) {
        st = load16(step_state + off);
        cmask = tmpl_cond_mask[tmpl];
    }
    wf_bytes16 now = st;
    const unsigned pend = look ? match16(st, WFS_PENDING) : 0u;   // bit j: step 16q+j
    // this lane's PENDING steps that carry a predicate and are not yet decided
    unsigned todo = pend & (unsigned)(cmask >> (q * 16)) & 0xffffu;
    unsigned long long setm = 0ull, clrm = 0ull;
    unsigned n_true = 0u, n_false = 0u;
    bool again = __any(todo != 0u);                 // wave-uniform
    while (again) {
        const unsigned sat16 = mask16(
            now, [](unsigned s) { return s == WFS_SUCCEEDED || s == WFS_SKIPPED; });
        const unsigned long long sat = quad_or((unsigned long long)sat16 << (q * 16));
        bool skipped = false;
#pragma unroll 1
        for (unsigned f = todo; f != 0u; f &= f - 1u) {
            const int j = __ffs((int)f) - 1;
            const size_t i = off + j;
            if (((unsigned long long)deps_mask[i] & ~sat) != 0ull) continue;
            todo &= ~(1u << j);
            const bool v = wf_cond_value(tmpl_cond[(size_t)tmpl * 64 + q * 16 + j],
                                         run_input + (size_t)r * IW, IW,
                                         step_out + (size_t)r * 64);
            n_true += v ? 1u : 0u;
            n_false += v ? 0u : 1u;
            if (step_kind[i] == WFK_CONDITION) {
                const unsigned long long bit = 1ull << (q * 16 + j);
                if (v) setm |= bit; else clrm |= bit;
                step_out[i] = v ? 1 : 0;
            } else if (!v) {
                set_byte(now, j, WFS_SKIPPED);
                skipped = true;
            }
        }
        // only a step skipped in this pass can have made another one ready
        again = __any(skipped) && __any(todo != 0u);
    }
    unsigned long long acc = 0ull;
    if (__any((setm | clrm) != 0ull || n_true + n_false != 0u)) {   // wave-uniform
        setm = quad_or(setm);
        clrm = quad_or(clrm);
        if (q == 0 && (setm | clrm) != 0ull)
            cond_bits[r] = (cond_bits[r] & ~clrm) | setm;
        store16_if_changed(step_state + off, now, st);
        // wave totals in one butterfly: two 32-bit fields (each <= 1024 per
        // wave, <= 4096 per block)
        acc = wave_sum((unsigned long long)n_true | (unsigned long long)n_false << 32);
    }
    const unsigned long long sum = block_sum(acc);
    if (threadIdx.x == 0) {
        const unsigned long long nt = sum & 0xffffffffull, nf = sum >> 32;
        if (nt) atomicAdd(&cond_counts[0], nt);
        if (nf) atomicAdd(&cond_counts[1], nf);
    }
}

// wf_child_payload runs after wf_expand and writes the payload row of every
// child emitted this tick (arena slots 0 .. min(child_count, CB) - 1):
//   words [0, IW)  the run's input words
//   word  IW       the child's emission ordinal (child_seq)
//   word  IW + 1   its step index
//   the rest       zero
// so a child's echo checksum is a function of (run input, step, ordinal) and
// of nothing else. The grid is fixed (graph capture), one wave per row and
// striding over the rows; the count is read from memory and nothing past it
// is touched.
__global__ __launch_bounds__(BLOCK) void wf_child_payload_kernel(
    const int* __restrict__ child_tag,              // [CB]
    const int* __restrict__ child_seq,              // [CB]
    const int* __restrict__ child_count,            // [1]
    const int* __restrict__ run_input,              // [NR*IW]
    int* __restrict__ child_payload,                // [CB*W]
    int CB, int NR, int IW, int W)
{
    const int n = min(max(*child_count, 0), CB);
    const int lane = threadIdx.x % WAVE;
    const int nwaves = (int)gridDim.x * (BLOCK / WAVE);
    // one wave per row: tag and ordinal are wave-uniform loads, the row is
    // written as consecutive words
    for (int c = blockIdx.x * (BLOCK / WAVE) + threadIdx.x / WAVE; c < n; c += nwaves) {
        const int tag = child_tag[c];
        const int seq = child_seq[c];
        const int run = tag >> 6;
        const bool known = (unsigned)run < (unsigned)NR;
        int* __restrict__ row = child_payload + (size_t)c * W;
        for (int k = lane; k < W; k += WAVE) {
            int v = 0;
            if (k < IW) v = known ? run_input[(size_t)run * IW + k] : 0;
            else if (k == IW) v = seq;
            else if (k == IW + 1) v = tag & 63;
            row[k] = v;
        }
    }
}

// ---------------------------------------------------------------------------
// K3-WF externally decided approvals: hold scan / hold list / decide
// ---------------------------------------------------------------------------
// With approvals decided from outside, an APPROVAL step that wf_sweep set
// WAITING stays WAITING until wf_decide names it by (slot, gen, step). The
// hold tables remember since when: hold_mask[r] bit s = step s has an open
// hold, hold_tick[r*64+s] = the tick it opened, hold_ttl[r*64+s] = ticks
// until it expires (0 = never). A row's hold data counts only while
//   hold_gen[r] == run_gen[r] && run_life[r] == LIVE && run_active[r] == 1;
// otherwise it is empty, whatever the words hold: a slot can be cancelled,
// drained and re-admitted between two ticks with no pass in between.
//
// wf_hold_scan runs inside the tick, directly after wf_sweep. Row-scan layout
// (see the helpers above K3); the four lanes of a row OR their 16 mask bits
// together and lane q == 0 owns the mask word. A wave with no WAITING byte,
// no open hold and no generation change does nothing more after the loads
// and writes nothing; it never touches hold_tick / hold_ttl, which are read
// only for a hold that continues. The tables after a pass are a pure
// function of the tables before it; the atomics are the cumulative counters
// (opened, expired) and the open-hold gauge, at most one add per block each.
//
// A hold opened at tick h with ttl T expires in the pass of tick h + T if it
// is still WAITING then: the step becomes FAILED, wf_status fails the run
// later in the same tick.
__global__ __launch_bounds__(BLOCK) void wf_hold_scan_kernel(
    unsigned char* __restrict__ step_state,         // [NR*64]
    const unsigned char* __restrict__ n_steps,      // [NR]
    const unsigned char* __restrict__ run_life,     // [NR]
    const unsigned char* __restrict__ run_active,   // [NR]
    const int* __restrict__ run_gen,                // [NR]
    const int* __restrict__ tick_p,
    const int* __restrict__ hold_ttl,               // [NR*64]
    unsigned long long* __restrict__ hold_mask,     // [NR]
    int* __restrict__ hold_tick,                    // [NR*64]
    int* __restrict__ hold_gen,                     // [NR]
    unsigned long long* __restrict__ hold_counts,   // [4] opened, expired, ...
    int* __restrict__ hold_open,                    // [1]
    int NR)
{
    const auto [r, q, off] = wf_row_coords();
    const int life = r < NR ? (int)run_life[r] : WFL_FREE;
    bool act = false, match = false;
    int gen = 0;
    unsigned long long raw = 0ull;                  // the mask word as stored
    unsigned wait = 0u;                             // bit j: step 16q+j is WAITING
    if (life != WFL_FREE) {
        gen = run_gen[r];
        match = hold_gen[r] == gen;
        raw = hold_mask[r];
        act = life == WFL_LIVE && run_active[r] == 1;
        // the states of a LIVE row are loaded with the narrow words above,
        // not after the active byte: one dependent round less for the rows
        // that matter, 64 bytes read in vain for a terminal, unreported one
        wf_bytes16 st = {};
        if (life == WFL_LIVE) st = load16(step_state + off);
        if (act) {
            wait = match16(st, WFS_WAITING);
            if (wait != 0u) {                       // bytes at s >= n_steps are no steps
                const int left = (int)n_steps[r] - q * 16;
                wait &= left >= 16 ? 0xffffu : left <= 0 ? 0u : (1u << left) - 1u;
            }
        }
    }
    const unsigned long long old = match ? raw : 0ull;   // the mask that counts
    // work: a WAITING step, an open hold to look at or to clear, or a row
    // admitted since its hold words were written. A wave without any skips
    // to the block's counter sum below.
    const bool busy = __any(wait != 0u || (match && raw != 0ull) || (act && !match));

    const int tick = *tick_p;
    const unsigned oldq = (unsigned)(old >> (q * 16)) & 0xffffu;
    unsigned keep = 0u;                             // this lane's 16 bits after the pass
    int opened = 0, expired = 0;
    if (busy && act) {
        const unsigned fresh = wait & ~oldq;
        unsigned cont = wait & oldq;
        keep = wait;
        opened = __popc(fresh);
#pragma unroll 1
        for (unsigned f = fresh; f != 0u; f &= f - 1u)
            hold_tick[off + (__ffs((int)f) - 1)] = tick;
#pragma unroll 1
        for (; cont != 0u; cont &= cont - 1u) {
            const int j = __ffs((int)cont) - 1;
            const int ttl = hold_ttl[off + j];
            if (ttl > 0 && tick - hold_tick[off + j] >= ttl) {
                step_state[off + j] = WFS_FAILED;
                keep &= ~(1u << j);
                ++expired;
            }
        }
    }
    unsigned long long acc = 0ull;
    if (busy) {                                     // wave-uniform
        // the row's new mask: OR of its four lanes' bits (lanes 4k .. 4k+3)
        const unsigned long long now = quad_or((unsigned long long)keep << (q * 16));
        int open = 0;
        if (q == 0 && life != WFL_FREE) {
            if (act) {
                if (now != raw) hold_mask[r] = now;
                if (!match) hold_gen[r] = gen;
                open = __popcll(now);
            } else if (match && raw != 0ull) {
                hold_mask[r] = 0ull;                // cancelled or finished with holds open
            }
        }
        // wave totals in one butterfly: three 21-bit fields (each <= 1024)
        acc = wave_sum((unsigned long long)opened | (unsigned long long)expired << 21
                       | (unsigned long long)open << 42);
    }
    const unsigned long long sum = block_sum(acc);
    if (threadIdx.x == 0) {
        const unsigned long long no = sum & 0x1fffffull, ne = (sum >> 21) & 0x1fffffull;
        const int nopen = (int)(sum >> 42);         // each field <= 4096
        if (no) atomicAdd(&hold_counts[0], no);
        if (ne) atomicAdd(&hold_counts[1], ne);
        if (nopen) atomicAdd(hold_open, nopen);
    }
}

// hold listing, pass 1 of 3 (between ticks): one thread per row. A row's
// listable holds are its valid mask bits whose step is still WAITING and
// whose key slot*64+step is at or after the cursor; only a row with a
// nonzero valid mask reads its states. The filtered mask is kept for the
// write pass (a snapshot, so both passes agree), its popcounts are summed
// per 256-row block for the scan (wf_admit_scan_kernel).
__global__ __launch_bounds__(BLOCK) void wf_hold_list_count_kernel(
    const unsigned char* __restrict__ step_state,   // [NR*64]
    const unsigned char* __restrict__ run_life,
    const unsigned char* __restrict__ run_active,
    const int* __restrict__ run_gen,
    const unsigned long long* __restrict__ hold_mask,
    const int* __restrict__ hold_gen,
    long long cursor,
    unsigned long long* __restrict__ list_mask,     // [NR] workspace
    int* __restrict__ blk_scan,                     // [nblk+1] counts, scanned next
    int NR)
{
    const int r = blockIdx.x * BLOCK + threadIdx.x;
    unsigned long long m = 0ull;
    if (r < NR) {
        if (run_life[r] == WFL_LIVE && run_active[r] == 1 && hold_gen[r] == run_gen[r])
            m = hold_mask[r];
        const long long key0 = (long long)r * 64;
        if (key0 + 63 < cursor) m = 0ull;
        else if (key0 < cursor) m &= ~0ull << (int)(cursor - key0);   // shift 1..63
        if (m != 0ull) {
            const unsigned char* row = step_state + (size_t)r * 64;
            unsigned long long w = 0ull;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                w |= (unsigned long long)match16(load16(row + k * 16), WFS_WAITING) << (k * 16);
            m &= w;
        }
        list_mask[r] = m;
    }
    const int n = block_sum(wave_sum((int)__popcll(m)));
    if (threadIdx.x == 0) blk_scan[blockIdx.x] = n;
}

// hold listing, pass 3: the ordered write. Row r's records start at the
// scanned count of its block plus the popcounts of the rows before it in
// the block, so positions ascend with (slot, step) and a full page holds
// exactly the cap lowest keys. list[0] = the number that matched.
__global__ __launch_bounds__(BLOCK) void wf_hold_list_write_kernel(
    const unsigned long long* __restrict__ list_mask,   // [NR]
    const int* __restrict__ blk_scan,               // [nblk+1] scanned
    const int* __restrict__ run_gen,
    const int* __restrict__ hold_tick,              // [NR*64]
    int* __restrict__ list,                         // [4 + cap*4]
    int NR, int nblk, int cap)
{
    __shared__ int wsum[BLOCK / WAVE];
    const int r = blockIdx.x * BLOCK + threadIdx.x;
    const int lane = threadIdx.x % WAVE;
    const int w = threadIdx.x / WAVE;
    unsigned long long m = r < NR ? list_mask[r] : 0ull;
    const int n = __popcll(m);
    const int incl = wave_prefix_sum(n, lane);
    if (lane == WAVE - 1) wsum[w] = incl;
    __syncthreads();
    int pos = blk_scan[blockIdx.x] + incl - n;
    for (int k = 0; k < w; ++k) pos += wsum[k];
    if (r == 0) list[0] = blk_scan[nblk];
    if (m == 0ull || pos >= cap) return;
    const int gen = run_gen[r];
    for (; m != 0ull && pos < cap; m &= m - 1ull, ++pos) {
        const int s = __ffsll((long long)m) - 1;
        *reinterpret_cast<int4*>(list + 4 + (size_t)pos * 4) =
            make_int4(r, gen, s, hold_tick[(size_t)r * 64 + s]);
    }
}

// decisions (between ticks): one thread per request, distinct (slot, step)
// pairs (the host sends only the first of a repeated pair). Result codes:
// 0 applied, 1 stale handle, 2 run no longer active, 3 not a waiting
// approval. It writes the one state byte; the next scan closes the hold and
// wf_hold_list already filters on the state.
__global__ __launch_bounds__(BLOCK) void wf_decide_kernel(
    const int* __restrict__ req_slot,               // [n]
    const int* __restrict__ req_gen,
    const int* __restrict__ req_step,
    const int* __restrict__ req_verdict,
    int n,
    const unsigned char* __restrict__ run_life,
    const int* __restrict__ run_gen,
    const unsigned char* __restrict__ run_active,
    const unsigned char* __restrict__ n_steps,
    const unsigned char* __restrict__ step_kind,    // [NR*64]
    unsigned char* __restrict__ step_state,         // [NR*64]
    unsigned long long* __restrict__ hold_counts,   // [4] ..., approved, rejected
    unsigned char* __restrict__ out_code,           // [n]
    int NR)
{
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    bool yes = false, no = false;
    if (i < n) {
        const int slot = req_slot[i], step = req_step[i];
        int code = 0;
        if (slot < 0 || slot >= NR || run_life[slot] != WFL_LIVE
            || run_gen[slot] != req_gen[i])
            code = 1;
        else if (run_active[slot] != 1)
            code = 2;
        else if (step < 0 || step >= (int)n_steps[slot]
                 || step_kind[(size_t)slot * 64 + step] != WFK_APPROVAL
                 || step_state[(size_t)slot * 64 + step] != WFS_WAITING)
            code = 3;
        if (code == 0) {
            yes = req_verdict[i] != 0;
            no = !yes;
            step_state[(size_t)slot * 64 + step] = yes ? WFS_SUCCEEDED : WFS_FAILED;
        }
        out_code[i] = (unsigned char)code;
    }
    // one add per counter and wave
    const unsigned long long ym = __ballot(yes), nm = __ballot(no);
    if (threadIdx.x % WAVE == 0) {
        if (ym) atomicAdd(&hold_counts[2], (unsigned long long)__popcll(ym));
        if (nm) atomicAdd(&hold_counts[3], (unsigned long long)__popcll(nm));
    }
}

// ---------------------------------------------------------------------------
// K4: deadline / staleness scan -> TIMEOUT candidates (compacted list)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void deadline_scan_kernel(
    const unsigned char* __restrict__ states,   // [N]
    const long long* __restrict__ deadlines,    // [N] unix micros
    const long long* __restrict__ updated_at,   // [N] unix micros
    long long now_us, long long dispatch_cutoff_us, long long running_cutoff_us,
    int* __restrict__ out_slots,                // [cap]
    int* __restrict__ out_count,                // [1]
    int N, int cap)
{
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= N) return;
    const unsigned char st = states[i];
    // active states: PENDING(1) APPROVAL(2) SCHEDULED(3) DISPATCHED(4) RUNNING(5)
    bool expired = false;
    if (st >= 1 && st <= 5 && deadlines[i] <= now_us) expired = true;
    if (st == 4 && updated_at[i] <= dispatch_cutoff_us) expired = true;  // DISPATCHED stale
    if (st == 5 && updated_at[i] <= running_cutoff_us) expired = true;   // RUNNING stale
    const int lane = threadIdx.x % WAVE;
    const int pos = wave_append_slot(expired, out_count, lane);
    if (pos >= 0 && pos < cap) out_slots[pos] = i;
}

// ---------------------------------------------------------------------------
// Echo worker: touch the job payload, write a result word, bump counters
// ---------------------------------------------------------------------------
// Payload arena: flat uint32 arena, job i owns [i*stride, (i+1)*stride).
// The "work" is a full read of the payload (the echo semantics: the result
// is derived from the entire context blob) + one result word per job.
__global__ __launch_bounds__(BLOCK) void echo_worker_kernel(
    const unsigned int* __restrict__ ctx_arena,  // [B*stride]
    unsigned int* __restrict__ res_arena,        // [B*stride]
    unsigned int* __restrict__ res_sum,          // [B]
    int B, int stride)
{
    // one wave per job, rows in batch order (echo_row)
    const int wave_id = (blockIdx.x * BLOCK + threadIdx.x) / WAVE;
    const int lane = threadIdx.x % WAVE;
    if (wave_id >= B) return;
    const size_t basep = (size_t)wave_id * stride;
    const unsigned int acc = echo_row(ctx_arena + basep, res_arena + basep, stride, lane);
    if (lane == 0) res_sum[wave_id] = acc;
}

__global__ __launch_bounds__(BLOCK) void echo_worker_indexed_kernel(
    const unsigned int* __restrict__ ctx_arena,  // [N*stride] home arena
    const int* __restrict__ slots,               // [B] job slots to execute
    unsigned int* __restrict__ res_arena,        // [N*stride] result arena
    unsigned int* __restrict__ res_sum,          // [N] by slot
    int B, int stride)
{
    // local-dispatch echo: read the job's payload in place (no staging copy
    // — within one GPU "dispatch" is just ownership, exactly as the worker
    // pool reads the HBM arena directly), write result + checksum.
    const int w = (blockIdx.x * BLOCK + threadIdx.x) / WAVE;
    const int lane = threadIdx.x % WAVE;
    if (w >= B) return;
    const int slot = slots[w];
    const size_t basep = (size_t)slot * stride;
    const unsigned int acc = echo_row(ctx_arena + basep, res_arena + basep, stride, lane);
    if (lane == 0) res_sum[slot] = acc;
}


// ---------------------------------------------------------------------------
// K1-MFMA: policy first-match on the matrix cores (comparison variant)
// ---------------------------------------------------------------------------
// One v_mfma_i32_16x16x64_i8 per dimension per 16-job x 16-rule tile computes
// all 256 set-intersection cardinalities of that dim at once. Epilogue turns
// the 9 dot products into the match predicate and reduces first-match per
// job across the 16 rule columns with 16-lane shuffles.
// See ops/policy_mfma.py for the fragment prepack and the measured
// bitset-vs-MFMA verdict.
typedef int v4i __attribute__((ext_vector_type(4)));

// The rule scan for TJ consecutive 16-job tiles held by one wave, shared by
// the kernels below, which differ only in where the lane's A fragments come
// from. With TJ > 1 one B-fragment load, one cards gather and one tile_dims
// read serve TJ MFMAs: the scan is bound by those dependent loads, not by
// the matrix cores (19 G int8 ops per tick are a few microseconds of MFMA).
template <int TJ>
__device__ __forceinline__ void mfma_first_match_tiles(
    const v4i (&afrag)[TJ][9],
    const signed char* __restrict__ b_pack,   // [Rt][9][64][16]
    const int* __restrict__ cards,            // [Rt*16][9]
    const signed char* __restrict__ rule_secrets, // [Rt*16]
    const unsigned char* __restrict__ job_secrets, // [J]
    const int* __restrict__ tile_dims,        // [Rt] bitmask of live dims
    int* __restrict__ out_first,              // [J] pre-filled INT_MAX
    int J, int R, int tiles_per_chunk)
{
    const int wave = threadIdx.x / WAVE;      // 4 waves per block
    const int lane = threadIdx.x % WAVE;
    const int jt0 = blockIdx.x * TJ;          // TJ job tiles per block
    const int Rt = (R + 15) / 16;
    const int chunk_begin = blockIdx.y * tiles_per_chunk;
    const int chunk_end = min(Rt, chunk_begin + tiles_per_chunk);

    const int row_base = (lane >> 4) * 4;     // 4 job rows per lane
    const int col = lane & 15;                // rule column
    int best[TJ][4];
    unsigned char jsec[TJ][4];
    #pragma unroll
    for (int t = 0; t < TJ; ++t) {
        #pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int job = (jt0 + t) * 16 + row_base + r;
            best[t][r] = INT_MAX;
            jsec[t][r] = (job < J) ? job_secrets[job] : 0;
        }
    }

    // early-exit checks only pay when each wave scans enough rule tiles
    const bool do_exit = (chunk_end - chunk_begin) > 32;

    for (int rt = chunk_begin + wave; rt < chunk_end; rt += 4) {
        // dim skipping: most rules constrain only 2-4 of the 9 set dims; a
        // dim whose card is 0 for EVERY rule in the tile auto-passes (any-of:
        // card==0 | _; all-of: 0==0), so its MFMA + B-fragment load is dead.
        // tile_dims is the per-tile union, uniform across the wave.
        const unsigned dmask = (unsigned)tile_dims[rt];
        const int rule = rt * 16 + col;
        const signed char rsec = rule_secrets[rule];
        bool ok[TJ][4];
        #pragma unroll
        for (int t = 0; t < TJ; ++t) {
            #pragma unroll
            for (int r = 0; r < 4; ++r) ok[t][r] = true;
        }
        #pragma unroll
        for (int d = 0; d < 9; ++d) {
            if (!(dmask & (1u << d))) continue;
            const v4i bfrag = *(const v4i*)&b_pack[(((size_t)rt * 9 + d) * 64 + lane) * 16];
            const int card = cards[rule * 9 + d];
            #pragma unroll
            for (int t = 0; t < TJ; ++t) {
                v4i zero = {0, 0, 0, 0};
                const v4i acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(afrag[t][d], bfrag, zero, 0, 0, 0);
                #pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (d < 7) ok[t][r] &= (card == 0) | (acc[r] > 0);   // any-of
                    else       ok[t][r] &= (acc[r] == card);             // all-of
                }
            }
        }
        #pragma unroll
        for (int t = 0; t < TJ; ++t) {
            #pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool pass = ok[t][r] & ((rsec < 0) | (rsec == (signed char)jsec[t][r]));
                if (pass && rule < R) best[t][r] = min(best[t][r], rule);
            }
        }

        // first-match early exit, adaptive: stop once every job row of the
        // tile has SOME match — later tiles only yield larger rule ids, and
        // a smaller id found by another wave/block wins at the atomicMin
        // anyway. Folding out_first (other blocks' published finds; the
        // value only decreases, so a stale read just skips less) pays only
        // when each wave scans many tiles: measured on the default config
        // (8 tiles/wave) ANY per-tile check loses (171.6 -> 145-167M
        // jobs/s), while at 16k rules (128 tiles/wave) the fold wins 35%+.
        // So: no checks on short scans, fold+ballot every 4th tile on long.
        if (do_exit && ((rt >> 2) & 3) == 3) {
            bool all_matched = true;
            #pragma unroll
            for (int t = 0; t < TJ; ++t) {
                #pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int job = (jt0 + t) * 16 + row_base + r;
                    if (job < J)
                        best[t][r] = min(best[t][r], __hip_atomic_load(&out_first[job],
                            __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
                    const unsigned long long m = __ballot(best[t][r] != INT_MAX);
                    all_matched &= ((m & 0xFFFFull) != 0) & (((m >> 16) & 0xFFFFull) != 0)
                                 & (((m >> 32) & 0xFFFFull) != 0) & (((m >> 48) & 0xFFFFull) != 0);
                }
            }
            if (all_matched) break;
        }
    }

    // min across the 16 rule columns (lanes sharing the same lane>>4 group)
    #pragma unroll
    for (int t = 0; t < TJ; ++t) {
        #pragma unroll
        for (int off = 8; off > 0; off >>= 1) {
            #pragma unroll
            for (int r = 0; r < 4; ++r)
                best[t][r] = min(best[t][r], __shfl_xor(best[t][r], off, WAVE));
        }
        if ((lane & 15) == 0) {
            #pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int job = (jt0 + t) * 16 + row_base + r;
                if (job < J && best[t][r] != INT_MAX) atomicMin(&out_first[job], best[t][r]);
            }
        }
    }
}

__global__ __launch_bounds__(BLOCK) void policy_first_match_mfma_kernel(
    const signed char* __restrict__ a_pack,   // [Jt][9][64][16]
    const signed char* __restrict__ b_pack,
    const int* __restrict__ cards,
    const signed char* __restrict__ rule_secrets,
    const unsigned char* __restrict__ job_secrets,
    const int* __restrict__ tile_dims,
    int* __restrict__ out_first,
    int J, int R, int tiles_per_chunk)
{
    const int lane = threadIdx.x % WAVE;
    const int jt = blockIdx.x;
    // A fragments for the 9 dims: lane-linear 16 B loads
    v4i afrag[1][9];
    #pragma unroll
    for (int d = 0; d < 9; ++d)
        afrag[0][d] = *(const v4i*)&a_pack[(((size_t)jt * 9 + d) * 64 + lane) * 16];
    mfma_first_match_tiles<1>(afrag, b_pack, cards, rule_secrets, job_secrets,
                              tile_dims, out_first, J, R, tiles_per_chunk);
}

// K1 straight from the staged bit words: each lane expands its own A
// fragments in registers (the bytes pack_jobs_mfma_kernel would have
// written: lane -> job row lane&15, 16-bit slice lane>>4 of the dim's word,
// one int8 per bit). Saves the pack launch and the write-then-read of the
// [Jt,9,64,16] pack (9.4 MB per tick at 16384 jobs) for 9 word loads.
// TJ = job tiles per wave (register blocking, see mfma_first_match_tiles).
template <int TJ>
__global__ __launch_bounds__(BLOCK) void policy_first_match_mfma_bits_kernel(
    const long long* __restrict__ any_bits,   // [J,7] (1-word vocab)
    const long long* __restrict__ all_bits,   // [J,2]
    const signed char* __restrict__ b_pack,
    const int* __restrict__ cards,
    const signed char* __restrict__ rule_secrets,
    const unsigned char* __restrict__ job_secrets,
    const int* __restrict__ tile_dims,
    int* __restrict__ out_first,
    int J, int R, int tiles_per_chunk)
{
    const int lane = threadIdx.x % WAVE;
    const int shift = (lane >> 4) * 16;
    v4i afrag[TJ][9];
    #pragma unroll
    for (int t = 0; t < TJ; ++t) {
        const int job = (blockIdx.x * TJ + t) * 16 + (lane & 15);
        #pragma unroll
        for (int d = 0; d < 9; ++d) {
            unsigned long long w = 0;
            if (job < J)
                w = (unsigned long long)(d < 7 ? any_bits[(size_t)job * 7 + d]
                                               : all_bits[(size_t)job * 2 + (d - 7)]);
            const unsigned int slice = (unsigned int)(w >> shift) & 0xFFFFu;
            // nibble -> 4 bytes of 0/1: the multiply puts bit b at 7b+b, the
            // mask keeps bit b of the nibble at byte b (little-endian =
            // element order)
            #pragma unroll
            for (int q = 0; q < 4; ++q)
                afrag[t][d][q] = (int)((((slice >> (4 * q)) & 0xFu) * 0x00204081u) & 0x01010101u);
        }
    }
    mfma_first_match_tiles<TJ>(afrag, b_pack, cards, rule_secrets, job_secrets,
                               tile_dims, out_first, J, R, tiles_per_chunk);
}

// K1 from compact rows: cols[J][L] holds one word per LIVE dimension (a
// dimension some rule constrains, ops/policy_mfma.py live_dims), so the
// staged batch carries L words per job instead of nine. col_map is the
// d -> column map, 4 bits per dimension, 0xF = no column: passed by value, so
// it is wave-uniform and part of the captured launch like R. A dimension
// without a column gets a zero fragment; the rule scan never looks at it
// (tile_dims has its bit clear in every tile, the binding checks that).
// With L == 0 nothing is read from cols. Only the word's source differs from
// the bits kernel; the expansion and the scan are the same.
template <int TJ>
__global__ __launch_bounds__(BLOCK) void policy_first_match_mfma_cols_kernel(
    const long long* __restrict__ cols,       // [J,L] (1-word vocab)
    int L, unsigned long long col_map,
    const signed char* __restrict__ b_pack,
    const int* __restrict__ cards,
    const signed char* __restrict__ rule_secrets,
    const unsigned char* __restrict__ job_secrets,
    const int* __restrict__ tile_dims,
    int* __restrict__ out_first,
    int J, int R, int tiles_per_chunk)
{
    const int lane = threadIdx.x % WAVE;
    const int shift = (lane >> 4) * 16;
    v4i afrag[TJ][9];
    #pragma unroll
    for (int t = 0; t < TJ; ++t) {
        const int job = (blockIdx.x * TJ + t) * 16 + (lane & 15);
        #pragma unroll
        for (int d = 0; d < 9; ++d) {
            const int c = (int)((col_map >> (4 * d)) & 0xFull);
            unsigned long long w = 0;
            if (c < L && job < J)
                w = (unsigned long long)cols[(size_t)job * L + c];
            const unsigned int slice = (unsigned int)(w >> shift) & 0xFFFFu;
            #pragma unroll
            for (int q = 0; q < 4; ++q)
                afrag[t][d][q] = (int)((((slice >> (4 * q)) & 0xFu) * 0x00204081u) & 0x01010101u);
        }
    }
    mfma_first_match_tiles<TJ>(afrag, b_pack, cards, rule_secrets, job_secrets,
                               tile_dims, out_first, J, R, tiles_per_chunk);
}

// ---------------------------------------------------------------------------
// Tick-fusion kernels: device-side compaction + count-pointer variants so a
// whole single-GPU control-plane tick is a fixed kernel sequence (no host
// syncs) and can be captured into a hipGraph (guide §Guideline 9).
// ---------------------------------------------------------------------------

// decisions gather + allow/deny split (replaces 6 torch glue ops)
__global__ __launch_bounds__(BLOCK) void policy_gate_kernel(
    const int* __restrict__ first,            // [J] first-match rule (-1 none)
    const signed char* __restrict__ decisions, // [R]
    signed char* __restrict__ out_decision,   // [J]
    int* __restrict__ denied_slots,           // [J] compacted
    int* __restrict__ denied_count,           // [1]
    int* __restrict__ allowed_slots,          // [J] compacted
    int* __restrict__ allowed_count,          // [1]
    int J, int R)
{
    const int j = blockIdx.x * BLOCK + threadIdx.x;
    const int lane = threadIdx.x % WAVE;
    gate_job(j, J, lane, first, decisions, R, out_decision,
             allowed_slots, allowed_count, denied_slots, denied_count);
}

// gate + DENIED transition + DLQ ring in ONE launch: the profile showed the
// split (gate, apply_transitions_dyn[DENIED], dlq_ring_append) spending
// ~14 us/tick on three ~4.6 us launches over the same denied set
// (profiles/r14_bench_ktrace_stats.txt) — at a 150 us tick that is pure
// launch-boundary tax (MI355X_MICROARCH.md price-list "kernel launch").
__global__ __launch_bounds__(BLOCK) void policy_gate_full_kernel(
    const int* __restrict__ first,            // [J]
    const signed char* __restrict__ decisions, // [R]
    signed char* __restrict__ out_decision,   // [J]
    int* __restrict__ denied_slots,           // [J] compacted
    int* __restrict__ denied_count,           // [1]
    int* __restrict__ allowed_slots,          // [J] compacted
    int* __restrict__ allowed_count,          // [1]
    unsigned char* __restrict__ states,
    long long* __restrict__ deadlines,
    int* __restrict__ dlq_ring,               // [ring_size]
    int* __restrict__ dlq_head,               // [1] monotonic
    int ring_size,
    int J, int R)
{
    const int j = blockIdx.x * BLOCK + threadIdx.x;
    const int lane = threadIdx.x % WAVE;
    const bool allowed = gate_job(j, J, lane, first, decisions, R, out_decision,
                                  allowed_slots, allowed_count, denied_slots, denied_count);
    deny_to_dlq(j < J && !allowed, j, lane, states, deadlines, dlq_ring, dlq_head, ring_size);
}

// tick prologue in one launch (begin_slot)
__global__ __launch_bounds__(BLOCK) void begin_tick_kernel(
    unsigned char* __restrict__ states, int B,
    int* __restrict__ counts, int ncounts,
    int* __restrict__ first)               // [B] primed for atomicMin, or null
{
    begin_slot(blockIdx.x * BLOCK + threadIdx.x, states, B, counts, ncounts, first);
}

// end-of-tick stats fold: the per-tick D2H counts read was the tick's only
// host sync (~15 us graph-replay + copy stall); accumulate on-device and let
// the host read ONCE per timed window instead
__global__ void accumulate_counts_kernel(
    const int* __restrict__ counts, long long* __restrict__ acc, int n)
{
    const int t = threadIdx.x;
    if (t < n) acc[t] += (long long)counts[t];
}

// routable compaction with the K2c spread computed inline: spread_pick keyed
// the round-robin on the slot index j, which this kernel already has — so a
// separate spread launch over all B slots was redundant work + launch tax
__global__ __launch_bounds__(BLOCK) void compact_routable_spread_kernel(
    const int* __restrict__ allowed_slots,    // [<=J]
    const int* __restrict__ allowed_count,    // [1]
    const int* __restrict__ pick,             // [J] exact least-loaded pick
    const int* __restrict__ order,            // [NW] workers by key asc
    const int* __restrict__ valid_count,      // [1] non-overloaded workers
    const long long* __restrict__ j_poolmask,
    const long long* __restrict__ j_labels,
    long long full_mask,
    int K,
    int* __restrict__ routable_slots,         // out
    int* __restrict__ routable_widx,          // out (global worker idx)
    int* __restrict__ routable_count)         // [1]
{
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    const int lane = threadIdx.x % WAVE;
    const bool live = i < *allowed_count;
    int j = 0, w = -1;
    if (live) {
        j = allowed_slots[i];
        w = route_pick(j, pick, order, valid_count, j_poolmask, j_labels, full_mask, K);
    }
    route_append(j, w, lane, routable_slots, routable_widx, routable_count);
}

// routable compaction: allowed jobs with a worker pick
__global__ __launch_bounds__(BLOCK) void compact_routable_kernel(
    const int* __restrict__ allowed_slots,    // [<=J]
    const int* __restrict__ allowed_count,    // [1]
    const int* __restrict__ pick,             // [J]
    int* __restrict__ routable_slots,         // out
    int* __restrict__ routable_widx,          // out (global worker idx)
    int* __restrict__ routable_count)         // [1]
{
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    const int lane = threadIdx.x % WAVE;
    const bool live = i < *allowed_count;
    int j = 0, w = -1;
    if (live) {
        j = allowed_slots[i];
        w = pick[j];
    }
    route_append(j, w, lane, routable_slots, routable_widx, routable_count);
}

// K5 with device-resident count + uniform target state
__global__ __launch_bounds__(BLOCK) void apply_transitions_dyn_kernel(
    unsigned char* __restrict__ states,
    int* __restrict__ attempts,
    long long* __restrict__ deadlines,
    const int* __restrict__ slots,
    const int* __restrict__ count,            // [1]
    unsigned char to)
{
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= *count) return;
    apply_one(states, attempts, deadlines, slots[i], to);
}

// chained K5 (march_chain): each routed slot through up to 4 states in ONE
// launch (SCHEDULED -> DISPATCHED -> RUNNING -> SUCCEEDED after the echo
// worker; the intermediate states are unobservable inside a captured graph,
// so four launches over the identical slot set were pure launch tax — see
// profiles/r14_bench_ktrace_stats.txt: apply_transitions_dyn 5x/tick, 13.6%).
// Also zeroes an extra int region (the per-tick local-load accumulator) so
// the load_feedback pass starts clean without its own zero_() launch.
__global__ __launch_bounds__(BLOCK) void apply_transitions_chain_dyn_kernel(
    unsigned char* __restrict__ states,
    int* __restrict__ attempts,
    long long* __restrict__ deadlines,
    const int* __restrict__ slots,
    const int* __restrict__ count,            // [1]
    int to0, int to1, int to2, int to3,       // -1 = unused
    int* __restrict__ extra_zero, int n_extra)
{
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < n_extra) extra_zero[i] = 0;
    if (i >= *count) return;
    const int chain[4] = {to0, to1, to2, to3};
    march_chain(states, attempts, deadlines, slots[i], chain);
}

__global__ __launch_bounds__(BLOCK) void echo_worker_indexed_dyn_kernel(
    const unsigned int* __restrict__ ctx_arena,
    const int* __restrict__ slots,
    const int* __restrict__ count,            // [1]
    unsigned int* __restrict__ res_arena,
    unsigned int* __restrict__ res_sum,
    int stride)
{
    const int w = (blockIdx.x * BLOCK + threadIdx.x) / WAVE;
    const int lane = threadIdx.x % WAVE;
    if (w >= *count) return;
    const int slot = slots[w];
    const size_t basep = (size_t)slot * stride;
    const unsigned int acc = echo_row(ctx_arena + basep, res_arena + basep, stride, lane);
    if (lane == 0) res_sum[slot] = acc;
}

// per-worker active-count histogram from the routable list: entries whose
// worker lives on this rank (wave_histogram_add)
__global__ __launch_bounds__(BLOCK) void load_feedback_kernel(
    const int* __restrict__ routable_widx,
    const int* __restrict__ count,
    int* __restrict__ w_active_local,         // [NWL] pre-zeroed
    int nwl, int my_rank)
{
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    const int lane = threadIdx.x % WAVE;
    bool live = i < *count;
    int bin = -1;
    if (live) {
        const int w = routable_widx[i];
        if (w / nwl == my_rank) bin = w % nwl;
        else live = false;
    }
    wave_histogram_add(live, bin, w_active_local, lane);
}

// ---------------------------------------------------------------------------
// Fused single-GPU tick: prologue | K2 pick | K1 | gate+route | finish.
// Ten of the old tick's twelve launches ran 4.4-8.8 us each over a few
// thousand threads of work (profiles/r49_e2e_overlap_ktrace_stats.txt):
// launch tax. The three kernels below call the same stage bodies as the
// per-stage kernels above (which the eager, padded and staged ticks still
// launch), several per launch. Sharing the bodies means the staged tick on
// the GPU no longer checks them; tests/test_gpu_tick_fusion.py also holds
// the fused tick to the staged tick on the CPU reference backend, which
// shares no code with this file.
// ---------------------------------------------------------------------------

// begin_tick_first + worker_precompute_into in one launch. w_key is written
// in full (the eager order refresh sorts it); `first` may be null.
__global__ __launch_bounds__(BLOCK) void tick_prologue_kernel(
    unsigned char* __restrict__ states, int B,
    int* __restrict__ counts, int ncounts,
    int* __restrict__ first,
    const int* __restrict__ w_active,
    const int* __restrict__ w_maxp,
    const float* __restrict__ w_cpu,
    const float* __restrict__ w_gpu,
    unsigned long long* __restrict__ w_key, int NW)
{
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    begin_slot(i, states, B, counts, ncounts, first);
    if (i < NW) w_key[i] = worker_key(i, w_active[i], w_maxp[i], w_cpu[i], w_gpu[i]);
}

// policy_gate_full + compact_routable_spread in one launch, one thread per
// job slot: decision, DENIED transition + DLQ append, allowed append, the
// spread / exact worker pick and the routable append. The compacted lists
// come out in a different (still unspecified) order; per-slot outputs are
// those of the two kernels it replaces. Also zeroes the per-tick local-load
// accumulator (the prologue has read it by now) for the finish kernel.
__global__ __launch_bounds__(BLOCK) void gate_route_kernel(
    const int* __restrict__ first,            // [J]
    const signed char* __restrict__ decisions, // [R]
    signed char* __restrict__ out_decision,   // [J]
    int* __restrict__ denied_slots, int* __restrict__ denied_count,
    int* __restrict__ allowed_slots, int* __restrict__ allowed_count,
    unsigned char* __restrict__ states,
    long long* __restrict__ deadlines,
    int* __restrict__ dlq_ring, int* __restrict__ dlq_head, int ring_size,
    const int* __restrict__ pick,             // [J] exact least-loaded pick
    const int* __restrict__ order,            // [NW] workers by key asc
    const int* __restrict__ valid_count,      // [1] non-overloaded workers
    const long long* __restrict__ j_poolmask,
    const long long* __restrict__ j_labels,
    long long full_mask, int K,
    int* __restrict__ routable_slots, int* __restrict__ routable_widx,
    int* __restrict__ routable_count,
    int* __restrict__ extra_zero, int n_extra,
    int J, int R)
{
    const int j = blockIdx.x * BLOCK + threadIdx.x;
    const int lane = threadIdx.x % WAVE;
    if (j < n_extra) extra_zero[j] = 0;
    const bool allowed = gate_job(j, J, lane, first, decisions, R, out_decision,
                                  allowed_slots, allowed_count, denied_slots, denied_count);
    deny_to_dlq(j < J && !allowed, j, lane, states, deadlines, dlq_ring, dlq_head, ring_size);
    int w = -1;
    if (allowed)
        w = route_pick(j, pick, order, valid_count, j_poolmask, j_labels, full_mask, K);
    route_append(j, w, lane, routable_slots, routable_widx, routable_count);
}

// echo_execute_indexed_dyn + apply_transitions_chain_dyn + load_feedback +
// accumulate_counts in one launch. routable_count is final before this
// kernel starts. One wave echoes one routed job and its lane 0 marches that
// job's state chain; thread i of the grid (there are 64 per routed job, so
// i < count is always covered) takes entry i of the load histogram with the
// same match-any aggregation as load_feedback_kernel; thread t < ncounts of
// block 0 folds the tick counters.
__global__ __launch_bounds__(BLOCK) void tick_finish_kernel(
    const unsigned int* __restrict__ ctx_arena,
    const int* __restrict__ slots,            // routable_slots
    const int* __restrict__ widx,             // routable_widx
    const int* __restrict__ count,            // [1] routable_count
    unsigned int* __restrict__ res_arena,
    unsigned int* __restrict__ res_sum,
    int stride,
    unsigned char* __restrict__ states,
    int* __restrict__ attempts,
    long long* __restrict__ deadlines,
    int to0, int to1, int to2, int to3,       // -1 = unused
    int* __restrict__ w_active_local,         // [NWL] zeroed by gate_route
    int nwl, int my_rank,
    const int* __restrict__ counts, long long* __restrict__ acc, int ncounts)
{
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    const int w = i / WAVE;
    const int lane = threadIdx.x % WAVE;
    const int n = *count;
    if (blockIdx.x == 0 && threadIdx.x < ncounts)
        acc[threadIdx.x] += (long long)counts[threadIdx.x];

    // load histogram: one thread per routed entry, grouped by equal bin
    bool live = i < n;
    int bin = -1;
    if (live) {
        const int wk = widx[i];
        if (wk / nwl == my_rank) bin = wk % nwl;
        else live = false;
    }
    wave_histogram_add(live, bin, w_active_local, lane);

    if (w >= n) return;  // wave-uniform
    const int slot = slots[w];
    const size_t basep = (size_t)slot * stride;
    const unsigned int sum = echo_row(ctx_arena + basep, res_arena + basep, stride, lane);
    if (lane == 0) {
        res_sum[slot] = sum;
        const int chain[4] = {to0, to1, to2, to3};
        march_chain(states, attempts, deadlines, slot, chain);
    }
}


// ---------------------------------------------------------------------------
// Padded cross-rank dispatch (multi-GPU path): fixed-capacity per-destination
// segments so the all_to_all shapes are static and the tick needs NO host
// splits sync. Capacity per destination = B (worst case: the whole batch to
// one rank); validity travels as a device-resident count vector.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void pack_by_dest_kernel(
    const int* __restrict__ routable_slots,   // [B]
    const int* __restrict__ routable_widx,    // [B] global worker idx
    const int* __restrict__ routable_count,   // [1]
    int* __restrict__ send_slots,             // [world*B]
    int* __restrict__ send_widx,              // [world*B] local worker idx
    int* __restrict__ send_cnt,               // [world] pre-zeroed
    int nwl, int cap,
    int* __restrict__ rq_src,                 // [rq_cap] requeue ring: slot (this batch)
    int* __restrict__ rq_widx,                // [rq_cap] global widx
    int* __restrict__ rq_attempts,            // [rq_cap] delivery attempts
    int* __restrict__ rq_count,               // [1]
    unsigned long long* __restrict__ rq_dead, // [1] dropped after max attempts / ring full
    int rq_cap,
    int* __restrict__ dead_src,               // [dead_cap] per-tick dead list (DLQ-bound)
    int* __restrict__ dead_count,             // [1] pre-zeroed per tick
    int dead_cap)
{
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    const int lane = threadIdx.x % WAVE;
    bool live = i < *routable_count;
    int slot = 0, widx = 0, dest = -1;
    if (live) {
        slot = routable_slots[i];
        widx = routable_widx[i];
        dest = widx / nwl;
    }
    // match-any aggregation on dest: one atomicAdd per distinct dest per wave
    unsigned long long pending = __ballot(live);
    int my_pos = -1;
    while (pending) {
        const int leader = __ffsll((long long)pending) - 1;
        const int leader_dest = __shfl(dest, leader, WAVE);
        const unsigned long long same = __ballot(live && dest == leader_dest);
        int base = 0;
        if (lane == leader) base = atomicAdd(&send_cnt[leader_dest], __popcll(same));
        base = __shfl(base, leader, WAVE);
        if (live && dest == leader_dest) {
            my_pos = base + __popcll(same & ((1ull << lane) - 1ull));
            live = false;
        }
        pending &= ~same;
    }
    if (my_pos < 0) return;
    if (my_pos < cap) {
        send_slots[(size_t)dest * cap + my_pos] = slot;
        send_widx[(size_t)dest * cap + my_pos] = widx % nwl;
    } else {
        // destination segment full: NAK-with-redelivery (bus/nats.go:146-168
        // analog) — park in the requeue ring, re-admitted next tick
        const int p = atomicAdd(rq_count, 1);
        if (p < rq_cap) {
            rq_src[p] = slot;      // payload row in this batch's home arena
            rq_widx[p] = widx;
            rq_attempts[p] = 1;
        } else {
            atomicAdd(rq_dead, 1ull);  // ring full -> DLQ-bound, counted
            const int dp = atomicAdd(dead_count, 1);
            if (dp < dead_cap) dead_src[dp] = slot;
        }
    }
}

// Redelivery pack: drain LAST tick's requeue ring into the padded send
// segments ahead of the fresh batch (redelivered jobs have priority, like
// a NAK'd message re-surfacing before new publishes). Entries that find
// their destination full again go back to the (new) requeue ring with
// attempts+1; past RQ_MAX_DELIVER they are dropped to rq_dead (the DLQ
// analog of JetStream max-deliver).
#define RQ_MAX_DELIVER 5
__global__ __launch_bounds__(BLOCK) void pack_requeue_kernel(
    const int* __restrict__ rq_prev_widx,     // [rq_cap]
    const int* __restrict__ rq_prev_attempts, // [rq_cap]
    const int* __restrict__ rq_prev_count,    // [1]
    int* __restrict__ send_slots,             // [world*cap]
    int* __restrict__ send_widx,              // [world*cap]
    int* __restrict__ send_cnt,               // [world] pre-zeroed
    int nwl, int cap,
    int* __restrict__ rq_src,
    int* __restrict__ rq_widx,
    int* __restrict__ rq_attempts,
    int* __restrict__ rq_count,
    unsigned long long* __restrict__ rq_dead,
    int rq_cap,
    int* __restrict__ dead_src,               // [dead_cap]
    int* __restrict__ dead_count,             // [1] pre-zeroed per tick
    int dead_cap)
{
    const int j = blockIdx.x * BLOCK + threadIdx.x;
    const int n = min(*rq_prev_count, rq_cap);
    if (j >= n) return;
    const int widx = rq_prev_widx[j];
    const int dest = widx / nwl;
    const int pos = atomicAdd(&send_cnt[dest], 1);
    if (pos < cap) {
        // flagged slot: payload comes from rq_prev_payload row j
        send_slots[(size_t)dest * cap + pos] = -1 - j;
        send_widx[(size_t)dest * cap + pos] = widx % nwl;
    } else {
        const int att = rq_prev_attempts[j] + 1;
        bool drop = att > RQ_MAX_DELIVER;
        if (!drop) {
            const int p = atomicAdd(rq_count, 1);
            if (p < rq_cap) {
                rq_src[p] = -1 - j;   // payload row in rq_prev_payload
                rq_widx[p] = widx;
                rq_attempts[p] = att;
            } else {
                drop = true;
            }
        }
        if (drop) {
            atomicAdd(rq_dead, 1ull);
            const int dp = atomicAdd(dead_count, 1);
            if (dp < dead_cap) dead_src[dp] = -1 - j;
        }
    }
}

// Materialize this tick's requeue-ring payloads into their own arena so the
// entries survive home-arena reuse (ring slots rotate every tick): source is
// the current batch (src >= 0) or last tick's rq arena (flagged).
__global__ __launch_bounds__(BLOCK) void materialize_rq_payload_kernel(
    const unsigned int* __restrict__ payload,         // [B*stride] this batch
    const unsigned int* __restrict__ rq_prev_payload, // [rq_cap*stride]
    const int* __restrict__ rq_src,                   // [rq_cap]
    const int* __restrict__ rq_count,                 // [1]
    unsigned int* __restrict__ rq_payload,            // [rq_cap*stride]
    int stride, int rq_cap)
{
    const int j = (blockIdx.x * BLOCK + threadIdx.x) / WAVE;
    const int lane = threadIdx.x % WAVE;
    const int n = min(*rq_count, rq_cap);
    if (j >= n) return;
    const int src = rq_src[j];
    const unsigned int* row = src >= 0 ? payload + (size_t)src * stride
                                       : rq_prev_payload + (size_t)(-1 - src) * stride;
    unsigned int* dst = rq_payload + (size_t)j * stride;
    for (int k = lane; k < stride; k += WAVE)
        dst[k] = row[k];
}

// gather payload rows into the padded send arena, region-valid; flagged
// (negative) slots are redeliveries whose payload lives in rq_prev_payload
__global__ __launch_bounds__(BLOCK) void gather_payload_padded_kernel(
    const unsigned int* __restrict__ payload,  // [B*stride] home arena
    const unsigned int* __restrict__ rq_prev_payload, // [rq_cap*stride]
    const int* __restrict__ send_slots,        // [world*cap]
    const int* __restrict__ send_cnt,          // [world]
    unsigned int* __restrict__ send_payload,   // [world*cap*stride]
    int stride, int cap, int world)
{
    const int w = (blockIdx.x * BLOCK + threadIdx.x) / WAVE;
    const int lane = threadIdx.x % WAVE;
    if (w >= world * cap) return;
    const int region = w / cap, e = w % cap;
    if (e >= send_cnt[region]) return;
    const int sslot = send_slots[w];
    const unsigned int* src = sslot >= 0
        ? payload + (size_t)sslot * stride
        : rq_prev_payload + (size_t)(-1 - sslot) * stride;
    const size_t dst = (size_t)w * stride;
    for (int k = lane; k < stride; k += WAVE)
        send_payload[dst + k] = src[k];
}

// region-valid echo over the padded receive arena
__global__ __launch_bounds__(BLOCK) void echo_padded_kernel(
    const unsigned int* __restrict__ recv_payload, // [world*cap*stride]
    const int* __restrict__ recv_cnt,              // [world]
    unsigned int* __restrict__ res_arena,          // [world*cap*stride]
    unsigned int* __restrict__ res_sums,           // [world*cap]
    int stride, int cap, int world)
{
    const int w = (blockIdx.x * BLOCK + threadIdx.x) / WAVE;
    const int lane = threadIdx.x % WAVE;
    if (w >= world * cap) return;
    const int region = w / cap, e = w % cap;
    if (e >= recv_cnt[region]) return;
    const size_t basep = (size_t)w * stride;
    const unsigned int acc = echo_row(recv_payload + basep, res_arena + basep, stride, lane);
    if (lane == 0) res_sums[w] = acc;
}

// region-valid transitions over the padded slot list
__global__ __launch_bounds__(BLOCK) void apply_transitions_padded_kernel(
    unsigned char* __restrict__ states,
    int* __restrict__ attempts,
    long long* __restrict__ deadlines,
    const int* __restrict__ slots_pad,        // [world*cap]
    const int* __restrict__ cnt,              // [world]
    unsigned char to, int cap, int world)
{
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= world * cap) return;
    if ((i % cap) >= cnt[i / cap]) return;
    const int slot = slots_pad[i];
    if (slot < 0) return;  // redelivered entry: its batch slot was recycled
    apply_one(states, attempts, deadlines, slot, to);
}

// region-valid per-worker load histogram from padded recv widx
__global__ __launch_bounds__(BLOCK) void load_feedback_padded_kernel(
    const int* __restrict__ recv_widx,        // [world*cap] local worker idx
    const int* __restrict__ recv_cnt,         // [world]
    int* __restrict__ w_active_local,         // [NWL] pre-zeroed
    int cap, int world)
{
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    const int lane = threadIdx.x % WAVE;
    const bool live = (i < world * cap) && ((i % cap) < recv_cnt[i / cap]);
    const int bin = live ? recv_widx[i] : -1;
    wave_histogram_add(live, bin, w_active_local, lane);
}

// ---------------------------------------------------------------------------
// Torch extension host wrappers
// ---------------------------------------------------------------------------

// device-side job packing for the MFMA K1 variant: bit words -> A-fragment
// layout (policy_mfma.py _pack_a semantics, byte-for-byte). One thread per
// (job-tile, dim, lane); each expands one 16-bit slice of the job's bit
// word into 16 int8 lanes. Lets the e2e ingest window run the MFMA kernel
// on freshly staged batches without a host packing pass.
__global__ __launch_bounds__(BLOCK) void pack_jobs_mfma_kernel(
    const long long* __restrict__ any_bits,   // [B,7] (1-word vocab)
    const long long* __restrict__ all_bits,   // [B,2]
    signed char* __restrict__ a_pack,         // [Jt,9,64,16]
    int B, int Jt)
{
    const int idx = blockIdx.x * BLOCK + threadIdx.x;
    if (idx >= Jt * 9 * 64) return;
    const int jt = idx / (9 * 64);
    const int rem = idx % (9 * 64);
    const int d = rem / 64;
    const int lane = rem % 64;
    const int row = lane & 15;
    const int kb = lane >> 4;
    const int job = jt * 16 + row;
    unsigned long long w = 0;
    if (job < B)
        w = (unsigned long long)(d < 7 ? any_bits[(size_t)job * 7 + d]
                                       : all_bits[(size_t)job * 2 + (d - 7)]);
    const unsigned int slice = (unsigned int)((w >> (kb * 16)) & 0xFFFFu);
    signed char* out = a_pack + (size_t)idx * 16;
    #pragma unroll
    for (int t = 0; t < 16; ++t)
        out[t] = (signed char)((slice >> t) & 1u);
}

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <array>

#include "synthetic_encode.h"

#define CHECK_DEV(t) TORCH_CHECK((t).is_cuda(), #t " must be on device")
#define CHECK_CONTIG(t) TORCH_CHECK((t).is_contiguous(), #t " must be contiguous")

static inline hipStream_t cur_stream() {
    return at::hip::getCurrentHIPStream().stream();
}

// Argument checks of the wf_* bindings; `op` is the binding's name, so every
// message starts with it. n is NR*64 for per-step tables, NR for per-run ones.
using wf_tensors = std::initializer_list<torch::Tensor>;

static void wf_check_numel(const char* op, int64_t n, wf_tensors tables) {
    for (const auto& t : tables) TORCH_CHECK(t.numel() == n, op, ": table sizes disagree");
}
static void wf_check_contiguous(const char* op, wf_tensors tables) {
    for (const auto& t : tables) TORCH_CHECK(t.is_contiguous(), op, ": tables must be contiguous");
}
// tables read or written with 16-byte vector accesses; `what` names them
static void wf_check_aligned16(const char* op, const char* what, wf_tensors tables) {
    for (const auto& t : tables)
        TORCH_CHECK((uintptr_t)t.data_ptr() % 16 == 0, op, ": ", what, " must be 16-byte aligned");
}
// the kernels index in int; n is the largest index a launch can form (a
// row-scan grid overshoots NR*64 by less than 1024)
static void wf_check_fits_int(const char* op, int64_t n) {
    TORCH_CHECK(n <= (int64_t)INT_MAX, op, ": table too large");
}
// grid of a row-scan kernel: 4 lanes per row
static int wf_row_grid(int64_t NR) { return (int)((NR * 4 + BLOCK - 1) / BLOCK); }

torch::Tensor policy_first_match(
    torch::Tensor rule_any, torch::Tensor rule_all, torch::Tensor rule_secrets,
    torch::Tensor rule_mcp, torch::Tensor rule_mcp_any,
    torch::Tensor job_any, torch::Tensor job_all, torch::Tensor job_secrets,
    torch::Tensor job_mcp, torch::Tensor job_mcp_used,
    int64_t rule_chunks)
{
    for (auto* t : {&rule_any, &rule_all, &rule_mcp, &job_any, &job_all, &job_mcp}) {
        CHECK_DEV(*t); CHECK_CONTIG(*t);
    }
    const int W = (int)rule_any.size(2);
    const int R = (int)rule_any.size(0);
    const int J = (int)job_any.size(0);
    TORCH_CHECK(job_any.size(2) == W, "word-count mismatch");
    auto out = torch::full({J}, INT_MAX,
        torch::TensorOptions().dtype(torch::kInt32).device(job_any.device()));
    if (R == 0 || J == 0) {
        return out.masked_fill(out == INT_MAX, -1);
    }
    // JPT: 2 jobs/thread halves the rule-stream traffic per block, but
    // measured NET-NEGATIVE at every shape tried (16k rules: 162->260 us;
    // 100k: 244->323 us — the doubled job-row registers cost occupancy and
    // the per-chunk early-out needs BOTH jobs finished). Kept selectable for
    // future shapes; disabled by measurement.
    const int JPT = 1;
    const int jobs_per_block = BLOCK * JPT;
    const int job_blocks = (J + jobs_per_block - 1) / jobs_per_block;
    int nchunks = (int)rule_chunks;
    if (nchunks <= 0) {
        nchunks = std::max(1, std::min((R + 511) / 512,
                                       std::max(1, 2048 / std::max(job_blocks, 1))));
    }
    const int per_chunk = (R + nchunks - 1) / nchunks;
    hipStream_t stream = cur_stream();

    auto launch = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(job_blocks, nchunks), dim3(BLOCK), 0, stream,
            (const long long*)rule_any.data_ptr<int64_t>(),
            (const long long*)rule_all.data_ptr<int64_t>(),
            (const signed char*)rule_secrets.data_ptr<int8_t>(),
            (const long long*)rule_mcp.data_ptr<int64_t>(),
            rule_mcp_any.data_ptr<uint8_t>(),
            (const long long*)job_any.data_ptr<int64_t>(),
            (const long long*)job_all.data_ptr<int64_t>(),
            job_secrets.data_ptr<uint8_t>(),
            (const long long*)job_mcp.data_ptr<int64_t>(),
            job_mcp_used.data_ptr<uint8_t>(),
            out.data_ptr<int>(), R, J, per_chunk);
    };
    if (JPT == 2) {
        switch (W) {
            case 1: launch(policy_first_match_kernel<1, 2>); break;
            case 2: launch(policy_first_match_kernel<2, 2>); break;
            case 4: launch(policy_first_match_kernel<4, 2>); break;
            default: TORCH_CHECK(false, "unsupported word count ", W);
        }
    } else {
        switch (W) {
            case 1: launch(policy_first_match_kernel<1, 1>); break;
            case 2: launch(policy_first_match_kernel<2, 1>); break;
            case 4: launch(policy_first_match_kernel<4, 1>); break;
            default: TORCH_CHECK(false, "unsupported word count ", W);
        }
    }
    out.masked_fill_(out == INT_MAX, -1);
    return out;
}

torch::Tensor worker_precompute(
    torch::Tensor w_pool, torch::Tensor w_active, torch::Tensor w_maxp,
    torch::Tensor w_cpu, torch::Tensor w_gpu)
{
    CHECK_DEV(w_pool);
    const int NW = (int)w_pool.size(0);
    auto keys = torch::empty({NW}, torch::TensorOptions().dtype(torch::kInt64).device(w_pool.device()));
    if (NW == 0) return keys;
    const int blocks = (NW + BLOCK - 1) / BLOCK;
    hipLaunchKernelGGL(worker_precompute_kernel, dim3(blocks), dim3(BLOCK), 0, cur_stream(),
        w_pool.data_ptr<int>(), w_active.data_ptr<int>(), w_maxp.data_ptr<int>(),
        w_cpu.data_ptr<float>(), w_gpu.data_ptr<float>(),
        (unsigned long long*)keys.data_ptr<int64_t>(), NW);
    return keys;
}

torch::Tensor least_loaded_pick(
    torch::Tensor w_pool, torch::Tensor w_keys, torch::Tensor w_labels,
    torch::Tensor j_poolmask, torch::Tensor j_labels)
{
    CHECK_DEV(w_pool); CHECK_DEV(j_poolmask);
    const int NW = (int)w_pool.size(0);
    const int NJ = (int)j_poolmask.size(0);
    auto out = torch::empty({NJ}, torch::TensorOptions().dtype(torch::kInt32).device(j_poolmask.device()));
    if (NJ == 0) return out;
    const int jobs_per_block = BLOCK / WAVE;
    const int blocks = (NJ + jobs_per_block - 1) / jobs_per_block;
    hipLaunchKernelGGL(least_loaded_pick_kernel, dim3(blocks), dim3(BLOCK), 0, cur_stream(),
        w_pool.data_ptr<int>(),
        (const unsigned long long*)w_keys.data_ptr<int64_t>(),
        (const long long*)w_labels.data_ptr<int64_t>(),
        (const long long*)j_poolmask.data_ptr<int64_t>(),
        (const long long*)j_labels.data_ptr<int64_t>(),
        out.data_ptr<int>(), NW, NJ, (const int*)nullptr, 0LL);
    return out;
}
void least_loaded_pick_into(
    torch::Tensor w_pool, torch::Tensor w_keys, torch::Tensor w_labels,
    torch::Tensor j_poolmask, torch::Tensor j_labels,
    torch::Tensor valid_count, int64_t full_mask, torch::Tensor out)
{
    CHECK_DEV(w_pool); CHECK_DEV(j_poolmask);
    const int NW = (int)w_pool.size(0);
    const int NJ = (int)j_poolmask.size(0);
    if (NJ == 0) return;
    const int jobs_per_block = BLOCK / WAVE;
    const int blocks = (NJ + jobs_per_block - 1) / jobs_per_block;
    hipLaunchKernelGGL(least_loaded_pick_kernel, dim3(blocks), dim3(BLOCK), 0, cur_stream(),
        w_pool.data_ptr<int>(),
        (const unsigned long long*)w_keys.data_ptr<int64_t>(),
        (const long long*)w_labels.data_ptr<int64_t>(),
        (const long long*)j_poolmask.data_ptr<int64_t>(),
        (const long long*)j_labels.data_ptr<int64_t>(),
        out.data_ptr<int>(), NW, NJ,
        valid_count.data_ptr<int>(), (long long)full_mask);
}

void dlq_ring_append(torch::Tensor slots, torch::Tensor count,
                     torch::Tensor ring, torch::Tensor head, int64_t capacity)
{
    const int blocks = ((int)capacity + BLOCK - 1) / BLOCK;
    hipLaunchKernelGGL(dlq_ring_append_kernel, dim3(blocks), dim3(BLOCK), 0, cur_stream(),
        slots.data_ptr<int>(), count.data_ptr<int>(), ring.data_ptr<int>(),
        head.data_ptr<int>(), (int)ring.size(0));
}

void worker_precompute_into(
    torch::Tensor w_pool, torch::Tensor w_active, torch::Tensor w_maxp,
    torch::Tensor w_cpu, torch::Tensor w_gpu, torch::Tensor out_keys)
{
    const int NW = (int)w_pool.size(0);
    if (NW == 0) return;
    const int blocks = (NW + BLOCK - 1) / BLOCK;
    hipLaunchKernelGGL(worker_precompute_kernel, dim3(blocks), dim3(BLOCK), 0, cur_stream(),
        w_pool.data_ptr<int>(), w_active.data_ptr<int>(), w_maxp.data_ptr<int>(),
        w_cpu.data_ptr<float>(), w_gpu.data_ptr<float>(),
        (unsigned long long*)out_keys.data_ptr<int64_t>(), NW);
}

void spread_pick(torch::Tensor order, torch::Tensor valid_count,
                 torch::Tensor j_poolmask, torch::Tensor j_labels,
                 int64_t full_mask, torch::Tensor pick, int64_t K)
{
    const int NJ = (int)pick.size(0);
    const int blocks = (NJ + BLOCK - 1) / BLOCK;
    hipLaunchKernelGGL(spread_pick_kernel, dim3(blocks), dim3(BLOCK), 0, cur_stream(),
        order.data_ptr<int>(), valid_count.data_ptr<int>(),
        (const long long*)j_poolmask.data_ptr<int64_t>(),
        (const long long*)j_labels.data_ptr<int64_t>(),
        (long long)full_mask, pick.data_ptr<int>(), NJ, (int)K);
}

void set_transition_lut(torch::Tensor lut) {
    TORCH_CHECK(lut.numel() == N_STATES * N_STATES, "lut must be 11x11");
    auto cpu = lut.to(torch::kUInt8).contiguous().cpu();
    (void)hipMemcpyToSymbol(HIP_SYMBOL(d_transition_lut), cpu.data_ptr<uint8_t>(),
                            N_STATES * N_STATES);
}

torch::Tensor apply_transitions(
    torch::Tensor states, torch::Tensor attempts, torch::Tensor deadlines,
    torch::Tensor slots, torch::Tensor to_states)
{
    CHECK_DEV(states); CHECK_DEV(slots);
    const int B = (int)slots.size(0);
    auto ok = torch::zeros({B}, torch::TensorOptions().dtype(torch::kUInt8).device(states.device()));
    if (B == 0) return ok;
    const int blocks = (B + BLOCK - 1) / BLOCK;
    hipLaunchKernelGGL(apply_transitions_kernel, dim3(blocks), dim3(BLOCK), 0, cur_stream(),
        states.data_ptr<uint8_t>(), attempts.data_ptr<int>(),
        slots.data_ptr<int>(), to_states.data_ptr<uint8_t>(),
        ok.data_ptr<uint8_t>(),
        (long long*)deadlines.data_ptr<int64_t>(), B);
    return ok;
}

std::tuple<torch::Tensor, torch::Tensor> deadline_scan(
    torch::Tensor states, torch::Tensor deadlines, torch::Tensor updated_at,
    int64_t now_us, int64_t dispatch_cutoff_us, int64_t running_cutoff_us, int64_t cap)
{
    CHECK_DEV(states);
    const int N = (int)states.size(0);
    auto slots = torch::empty({cap}, torch::TensorOptions().dtype(torch::kInt32).device(states.device()));
    auto count = torch::zeros({1}, torch::TensorOptions().dtype(torch::kInt32).device(states.device()));
    if (N == 0) return {slots, count};
    const int blocks = (N + BLOCK - 1) / BLOCK;
    hipLaunchKernelGGL(deadline_scan_kernel, dim3(blocks), dim3(BLOCK), 0, cur_stream(),
        states.data_ptr<uint8_t>(),
        (const long long*)deadlines.data_ptr<int64_t>(),
        (const long long*)updated_at.data_ptr<int64_t>(),
        (long long)now_us, (long long)dispatch_cutoff_us, (long long)running_cutoff_us,
        slots.data_ptr<int>(), count.data_ptr<int>(), N, (int)cap);
    return {slots, count};
}

torch::Tensor echo_execute(torch::Tensor ctx_arena, torch::Tensor res_arena, int64_t stride)
{
    CHECK_DEV(ctx_arena); CHECK_CONTIG(ctx_arena);
    const int B = (int)(ctx_arena.numel() / stride);
    auto sums = torch::empty({B}, torch::TensorOptions().dtype(torch::kInt32).device(ctx_arena.device()));
    const int waves_per_block = BLOCK / WAVE;
    const int blocks = (B + waves_per_block - 1) / waves_per_block;
    hipLaunchKernelGGL(echo_worker_kernel, dim3(blocks), dim3(BLOCK), 0, cur_stream(),
        (const unsigned int*)ctx_arena.data_ptr<int32_t>(),
        (unsigned int*)res_arena.data_ptr<int32_t>(),
        (unsigned int*)sums.data_ptr<int32_t>(), B, (int)stride);
    return sums;
}

torch::Tensor echo_execute_indexed(torch::Tensor ctx_arena, torch::Tensor slots,
                                   torch::Tensor res_arena, torch::Tensor res_sum,
                                   int64_t stride)
{
    CHECK_DEV(ctx_arena); CHECK_DEV(slots);
    const int B = (int)slots.size(0);
    if (B == 0) return res_sum;
    const int waves_per_block = BLOCK / WAVE;
    const int blocks = (B + waves_per_block - 1) / waves_per_block;
    hipLaunchKernelGGL(echo_worker_indexed_kernel, dim3(blocks), dim3(BLOCK), 0, cur_stream(),
        (const unsigned int*)ctx_arena.data_ptr<int32_t>(),
        slots.data_ptr<int>(),
        (unsigned int*)res_arena.data_ptr<int32_t>(),
        (unsigned int*)res_sum.data_ptr<int32_t>(), B, (int)stride);
    return res_sum;
}

torch::Tensor policy_first_match_mfma(
    torch::Tensor a_pack, torch::Tensor b_pack, torch::Tensor cards,
    torch::Tensor rule_secrets, torch::Tensor job_secrets,
    torch::Tensor tile_dims, int64_t n_jobs, int64_t n_rules)
{
    CHECK_DEV(a_pack); CHECK_DEV(b_pack);
    const int J = (int)n_jobs, R = (int)n_rules;
    const int Jt = (int)a_pack.size(0);
    const int Rt = (R + 15) / 16;
    auto out = torch::full({J}, INT_MAX,
        torch::TensorOptions().dtype(torch::kInt32).device(a_pack.device()));
    if (J == 0 || R == 0) return out.masked_fill_(out == INT_MAX, -1);
    // fill the chip: >=2048 workgroups via rule chunking
    int nchunks = std::max(1, std::min((Rt + 3) / 4, std::max(1, 2048 / std::max(Jt, 1))));
    const int tiles_per_chunk = (Rt + nchunks - 1) / nchunks;
    hipLaunchKernelGGL(policy_first_match_mfma_kernel, dim3(Jt, nchunks), dim3(BLOCK), 0, cur_stream(),
        (const signed char*)a_pack.data_ptr<int8_t>(),
        (const signed char*)b_pack.data_ptr<int8_t>(),
        cards.data_ptr<int>(),
        (const signed char*)rule_secrets.data_ptr<int8_t>(),
        job_secrets.data_ptr<uint8_t>(),
        tile_dims.data_ptr<int>(),
        out.data_ptr<int>(), J, R, tiles_per_chunk);
    out.masked_fill_(out == INT_MAX, -1);
    return out;
}

void policy_gate(torch::Tensor first, torch::Tensor decisions, torch::Tensor out_decision,
                 torch::Tensor denied_slots, torch::Tensor denied_count,
                 torch::Tensor allowed_slots, torch::Tensor allowed_count)
{
    const int J = (int)first.size(0);
    const int blocks = (J + BLOCK - 1) / BLOCK;
    hipLaunchKernelGGL(policy_gate_kernel, dim3(blocks), dim3(BLOCK), 0, cur_stream(),
        first.data_ptr<int>(), (const signed char*)decisions.data_ptr<int8_t>(),
        (signed char*)out_decision.data_ptr<int8_t>(),
        denied_slots.data_ptr<int>(), denied_count.data_ptr<int>(),
        allowed_slots.data_ptr<int>(), allowed_count.data_ptr<int>(),
        J, (int)decisions.size(0));
}

void compact_routable(torch::Tensor allowed_slots, torch::Tensor allowed_count,
                      torch::Tensor pick, torch::Tensor routable_slots,
                      torch::Tensor routable_widx, torch::Tensor routable_count)
{
    const int J = (int)pick.size(0);
    const int blocks = (J + BLOCK - 1) / BLOCK;
    hipLaunchKernelGGL(compact_routable_kernel, dim3(blocks), dim3(BLOCK), 0, cur_stream(),
        allowed_slots.data_ptr<int>(), allowed_count.data_ptr<int>(),
        pick.data_ptr<int>(), routable_slots.data_ptr<int>(),
        routable_widx.data_ptr<int>(), routable_count.data_ptr<int>());
}

void policy_gate_full(torch::Tensor first, torch::Tensor decisions, torch::Tensor out_decision,
                      torch::Tensor denied_slots, torch::Tensor denied_count,
                      torch::Tensor allowed_slots, torch::Tensor allowed_count,
                      torch::Tensor states, torch::Tensor deadlines,
                      torch::Tensor dlq_ring, torch::Tensor dlq_head)
{
    const int J = (int)first.size(0);
    const int blocks = (J + BLOCK - 1) / BLOCK;
    hipLaunchKernelGGL(policy_gate_full_kernel, dim3(blocks), dim3(BLOCK), 0, cur_stream(),
        first.data_ptr<int>(), (const signed char*)decisions.data_ptr<int8_t>(),
        (signed char*)out_decision.data_ptr<int8_t>(),
        denied_slots.data_ptr<int>(), denied_count.data_ptr<int>(),
        allowed_slots.data_ptr<int>(), allowed_count.data_ptr<int>(),
        states.data_ptr<uint8_t>(), (long long*)deadlines.data_ptr<int64_t>(),
        dlq_ring.data_ptr<int>(), dlq_head.data_ptr<int>(),
        (int)dlq_ring.size(0), J, (int)decisions.size(0));
}
void accumulate_counts(torch::Tensor counts, torch::Tensor acc)
{
    const int n = (int)counts.size(0);
    hipLaunchKernelGGL(accumulate_counts_kernel, dim3(1), dim3(WAVE), 0, cur_stream(),
        counts.data_ptr<int>(), (long long*)acc.data_ptr<int64_t>(), n);
}
static void launch_begin_tick(torch::Tensor& states, torch::Tensor& counts, int* first)
{
    const int B = (int)states.size(0);
    const int n = (int)counts.size(0);
    const int blocks = (std::max(B, n) + BLOCK - 1) / BLOCK;
    hipLaunchKernelGGL(begin_tick_kernel, dim3(blocks), dim3(BLOCK), 0, cur_stream(),
        states.data_ptr<uint8_t>(), B, counts.data_ptr<int>(), n, first);
}
void begin_tick(torch::Tensor states, torch::Tensor counts)
{
    launch_begin_tick(states, counts, nullptr);
}
void begin_tick_first(torch::Tensor states, torch::Tensor counts, torch::Tensor first)
{
    launch_begin_tick(states, counts, first.data_ptr<int>());
}
void policy_first_match_mfma_into(
    torch::Tensor a_pack, torch::Tensor b_pack, torch::Tensor cards,
    torch::Tensor rule_secrets, torch::Tensor job_secrets,
    torch::Tensor tile_dims, int64_t n_jobs, int64_t n_rules, torch::Tensor out)
{
    CHECK_DEV(a_pack); CHECK_DEV(b_pack);
    const int J = (int)n_jobs, R = (int)n_rules;
    const int Jt = (int)a_pack.size(0);
    const int Rt = (R + 15) / 16;
    if (J == 0 || R == 0) return;
    int nchunks = std::max(1, std::min((Rt + 3) / 4, std::max(1, 2048 / std::max(Jt, 1))));
    const int tiles_per_chunk = (Rt + nchunks - 1) / nchunks;
    hipLaunchKernelGGL(policy_first_match_mfma_kernel, dim3(Jt, nchunks), dim3(BLOCK), 0, cur_stream(),
        (const signed char*)a_pack.data_ptr<int8_t>(),
        (const signed char*)b_pack.data_ptr<int8_t>(),
        cards.data_ptr<int>(),
        (const signed char*)rule_secrets.data_ptr<int8_t>(),
        job_secrets.data_ptr<uint8_t>(),
        tile_dims.data_ptr<int>(),
        out.data_ptr<int>(), J, R, tiles_per_chunk);
}
void compact_routable_spread(torch::Tensor allowed_slots, torch::Tensor allowed_count,
                             torch::Tensor pick, torch::Tensor order, torch::Tensor valid_count,
                             torch::Tensor j_poolmask, torch::Tensor j_labels,
                             int64_t full_mask, int64_t K,
                             torch::Tensor routable_slots, torch::Tensor routable_widx,
                             torch::Tensor routable_count)
{
    const int J = (int)allowed_slots.size(0);
    const int blocks = (J + BLOCK - 1) / BLOCK;
    hipLaunchKernelGGL(compact_routable_spread_kernel, dim3(blocks), dim3(BLOCK), 0, cur_stream(),
        allowed_slots.data_ptr<int>(), allowed_count.data_ptr<int>(),
        pick.data_ptr<int>(), order.data_ptr<int>(), valid_count.data_ptr<int>(),
        (const long long*)j_poolmask.data_ptr<int64_t>(),
        (const long long*)j_labels.data_ptr<int64_t>(),
        (long long)full_mask, (int)K,
        routable_slots.data_ptr<int>(), routable_widx.data_ptr<int>(),
        routable_count.data_ptr<int>());
}
// a K5 chain as the kernels take it: four target states, -1 = unused
static std::array<int, 4> unpack_chain(const std::vector<int64_t>& chain)
{
    std::array<int, 4> to = {-1, -1, -1, -1};
    for (size_t c = 0; c < chain.size() && c < 4; ++c) to[c] = (int)chain[c];
    return to;
}
void apply_transitions_chain_dyn(torch::Tensor states, torch::Tensor attempts,
                                 torch::Tensor deadlines, torch::Tensor slots,
                                 torch::Tensor count, std::vector<int64_t> chain,
                                 torch::Tensor extra_zero, int64_t capacity)
{
    const auto to = unpack_chain(chain);
    const int n_extra = (int)extra_zero.size(0);
    const int blocks = (std::max((int)capacity, n_extra) + BLOCK - 1) / BLOCK;
    hipLaunchKernelGGL(apply_transitions_chain_dyn_kernel, dim3(blocks), dim3(BLOCK), 0, cur_stream(),
        states.data_ptr<uint8_t>(), attempts.data_ptr<int>(),
        (long long*)deadlines.data_ptr<int64_t>(),
        slots.data_ptr<int>(), count.data_ptr<int>(),
        to[0], to[1], to[2], to[3],
        extra_zero.data_ptr<int>(), n_extra);
}
void apply_transitions_dyn(torch::Tensor states, torch::Tensor attempts, torch::Tensor deadlines,
                           torch::Tensor slots, torch::Tensor count, int64_t to_state, int64_t capacity)
{
    const int blocks = ((int)capacity + BLOCK - 1) / BLOCK;
    hipLaunchKernelGGL(apply_transitions_dyn_kernel, dim3(blocks), dim3(BLOCK), 0, cur_stream(),
        states.data_ptr<uint8_t>(), attempts.data_ptr<int>(),
        (long long*)deadlines.data_ptr<int64_t>(),
        slots.data_ptr<int>(), count.data_ptr<int>(), (unsigned char)to_state);
}

void echo_execute_indexed_dyn(torch::Tensor ctx_arena, torch::Tensor slots, torch::Tensor count,
                              torch::Tensor res_arena, torch::Tensor res_sum,
                              int64_t stride, int64_t capacity)
{
    const int waves_per_block = BLOCK / WAVE;
    const int blocks = ((int)capacity + waves_per_block - 1) / waves_per_block;
    hipLaunchKernelGGL(echo_worker_indexed_dyn_kernel, dim3(blocks), dim3(BLOCK), 0, cur_stream(),
        (const unsigned int*)ctx_arena.data_ptr<int32_t>(), slots.data_ptr<int>(),
        count.data_ptr<int>(), (unsigned int*)res_arena.data_ptr<int32_t>(),
        (unsigned int*)res_sum.data_ptr<int32_t>(), (int)stride);
}

void load_feedback(torch::Tensor routable_widx, torch::Tensor count,
                   torch::Tensor w_active_local, int64_t nwl, int64_t my_rank, int64_t capacity)
{
    const int blocks = ((int)capacity + BLOCK - 1) / BLOCK;
    hipLaunchKernelGGL(load_feedback_kernel, dim3(blocks), dim3(BLOCK), 0, cur_stream(),
        routable_widx.data_ptr<int>(), count.data_ptr<int>(),
        w_active_local.data_ptr<int>(), (int)nwl, (int)my_rank);
}

// -- fused single-GPU tick (5 launches: these four + least_loaded_pick_into) --
void tick_prologue(torch::Tensor states, torch::Tensor counts,
                   c10::optional<torch::Tensor> first,
                   torch::Tensor w_active, torch::Tensor w_maxp,
                   torch::Tensor w_cpu, torch::Tensor w_gpu, torch::Tensor out_keys)
{
    CHECK_DEV(states);
    const int B = (int)states.size(0);
    const int n = (int)counts.size(0);
    const int NW = (int)out_keys.size(0);
    TORCH_CHECK(w_active.size(0) == NW && w_maxp.size(0) == NW &&
                w_cpu.size(0) == NW && w_gpu.size(0) == NW, "worker table size mismatch");
    TORCH_CHECK(!first.has_value() || first->size(0) == B, "first must be [B]");
    const int blocks = (std::max(std::max(B, n), std::max(NW, 1)) + BLOCK - 1) / BLOCK;
    hipLaunchKernelGGL(tick_prologue_kernel, dim3(blocks), dim3(BLOCK), 0, cur_stream(),
        states.data_ptr<uint8_t>(), B, counts.data_ptr<int>(), n,
        first.has_value() ? first->data_ptr<int>() : (int*)nullptr,
        w_active.data_ptr<int>(), w_maxp.data_ptr<int>(),
        w_cpu.data_ptr<float>(), w_gpu.data_ptr<float>(),
        (unsigned long long*)out_keys.data_ptr<int64_t>(), NW);
}

void policy_first_match_mfma_bits_into(
    torch::Tensor any_bits, torch::Tensor all_bits,
    torch::Tensor b_pack, torch::Tensor cards,
    torch::Tensor rule_secrets, torch::Tensor job_secrets,
    torch::Tensor tile_dims, int64_t n_rules, torch::Tensor out, int64_t job_tiles)
{
    CHECK_DEV(any_bits); CHECK_DEV(b_pack);
    CHECK_CONTIG(any_bits); CHECK_CONTIG(all_bits);
    TORCH_CHECK(job_tiles == 1 || job_tiles == 2, "job_tiles must be 1 or 2");
    TORCH_CHECK(any_bits.dim() == 3 && any_bits.size(1) == 7 && any_bits.size(2) == 1 &&
                all_bits.dim() == 3 && all_bits.size(1) == 2 && all_bits.size(2) == 1,
                "MFMA K1 needs the 1-word vocab: any [J,7,1], all [J,2,1]");
    const int J = (int)any_bits.size(0), R = (int)n_rules;
    TORCH_CHECK(all_bits.size(0) == J && job_secrets.size(0) >= J && out.size(0) >= J,
                "job tensors must cover J");
    const int TJ = (int)job_tiles;
    const int Jt = ((J + 15) / 16 + TJ - 1) / TJ;   // blocks of TJ job tiles
    const int Rt = (R + 15) / 16;
    if (J == 0 || R == 0) return;
    TORCH_CHECK(b_pack.size(0) >= Rt && tile_dims.size(0) >= Rt &&
                rule_secrets.size(0) >= Rt * 16 && cards.size(0) >= Rt * 16,
                "rule pack smaller than n_rules");
    int nchunks = std::max(1, std::min((Rt + 3) / 4, std::max(1, 2048 / std::max(Jt, 1))));
    const int tiles_per_chunk = (Rt + nchunks - 1) / nchunks;
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(Jt, nchunks), dim3(BLOCK), 0, cur_stream(),
            (const long long*)any_bits.data_ptr<int64_t>(),
            (const long long*)all_bits.data_ptr<int64_t>(),
            (const signed char*)b_pack.data_ptr<int8_t>(),
            cards.data_ptr<int>(),
            (const signed char*)rule_secrets.data_ptr<int8_t>(),
            job_secrets.data_ptr<uint8_t>(),
            tile_dims.data_ptr<int>(),
            out.data_ptr<int>(), J, R, tiles_per_chunk);
    };
    // 4 tiles per wave was tried and dropped: 215 VGPRs, 2 waves/SIMD, 41 us
    // against 27 us for 2 (profiles/r51_k1_register_blocking.txt)
    if (TJ == 2) launch(policy_first_match_mfma_bits_kernel<2>);
    else launch(policy_first_match_mfma_bits_kernel<1>);
}

// K1 from compact rows (policy_first_match_mfma_cols_kernel). The checks of
// the bits variant, plus the ones that keep a stale column map loud: the map
// must name exactly the columns 0..L-1, ascending in d, and every dimension
// some rule tile scans must have a column. tile_dims lives on the device, so
// that last check reads it back: not possible (and not needed) while the
// stream is being captured, where the call repeats an eager warm-up call
// with the same arguments that was checked.
void policy_first_match_mfma_cols_into(
    torch::Tensor cols, int64_t col_map,
    torch::Tensor b_pack, torch::Tensor cards,
    torch::Tensor rule_secrets, torch::Tensor job_secrets,
    torch::Tensor tile_dims, int64_t n_rules, torch::Tensor out, int64_t job_tiles)
{
    CHECK_DEV(cols); CHECK_DEV(b_pack);
    CHECK_CONTIG(cols);
    TORCH_CHECK(job_tiles == 1 || job_tiles == 2, "job_tiles must be 1 or 2");
    TORCH_CHECK(cols.dim() == 2 && cols.scalar_type() == torch::kInt64 && cols.size(1) <= 9,
                "compact K1 needs cols [J,L] int64 with L <= 9 (1-word vocab)");
    const int J = (int)cols.size(0), R = (int)n_rules, L = (int)cols.size(1);
    TORCH_CHECK(job_secrets.size(0) >= J && out.size(0) >= J, "job tensors must cover J");
    TORCH_CHECK(col_map >= 0 && (col_map >> 36) == 0, "col_map holds 9 nibbles");
    unsigned map_dims = 0;
    int next_col = 0;
    for (int d = 0; d < 9; ++d) {
        const int c = (int)((col_map >> (4 * d)) & 0xF);
        if (c == 0xF) continue;
        TORCH_CHECK(c == next_col, "col_map must number the live dims 0..L-1 in ascending d");
        ++next_col;
        map_dims |= 1u << d;
    }
    TORCH_CHECK(next_col == L, "col_map names ", next_col, " columns, cols has ", L);
    const int TJ = (int)job_tiles;
    const int Jt = ((J + 15) / 16 + TJ - 1) / TJ;   // blocks of TJ job tiles
    const int Rt = (R + 15) / 16;
    if (J == 0 || R == 0) return;
    TORCH_CHECK(b_pack.size(0) >= Rt && tile_dims.size(0) >= Rt &&
                rule_secrets.size(0) >= Rt * 16 && cards.size(0) >= Rt * 16,
                "rule pack smaller than n_rules");
    hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
    TORCH_CHECK(hipStreamIsCapturing(cur_stream(), &capturing) == hipSuccess,
                "hipStreamIsCapturing failed");
    if (capturing == hipStreamCaptureStatusNone) {
        const torch::Tensor td = tile_dims.narrow(0, 0, Rt).cpu();
        const int* p = td.data_ptr<int>();
        unsigned scanned = 0;
        for (int rt = 0; rt < Rt; ++rt) scanned |= (unsigned)p[rt];
        TORCH_CHECK((scanned & 0x1FFu & ~map_dims) == 0,
                    "col_map lacks a dimension the packed policy scans (stale map?): "
                    "tile_dims union ", scanned & 0x1FFu, ", map dims ", map_dims);
    }
    int nchunks = std::max(1, std::min((Rt + 3) / 4, std::max(1, 2048 / std::max(Jt, 1))));
    const int tiles_per_chunk = (Rt + nchunks - 1) / nchunks;
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(Jt, nchunks), dim3(BLOCK), 0, cur_stream(),
            (const long long*)cols.data_ptr<int64_t>(), L, (unsigned long long)col_map,
            (const signed char*)b_pack.data_ptr<int8_t>(),
            cards.data_ptr<int>(),
            (const signed char*)rule_secrets.data_ptr<int8_t>(),
            job_secrets.data_ptr<uint8_t>(),
            tile_dims.data_ptr<int>(),
            out.data_ptr<int>(), J, R, tiles_per_chunk);
    };
    if (TJ == 2) launch(policy_first_match_mfma_cols_kernel<2>);
    else launch(policy_first_match_mfma_cols_kernel<1>);
}

void gate_route(torch::Tensor first, torch::Tensor decisions, torch::Tensor out_decision,
                torch::Tensor denied_slots, torch::Tensor denied_count,
                torch::Tensor allowed_slots, torch::Tensor allowed_count,
                torch::Tensor states, torch::Tensor deadlines,
                torch::Tensor dlq_ring, torch::Tensor dlq_head,
                torch::Tensor pick, torch::Tensor order, torch::Tensor valid_count,
                torch::Tensor j_poolmask, torch::Tensor j_labels,
                int64_t full_mask, int64_t K,
                torch::Tensor routable_slots, torch::Tensor routable_widx,
                torch::Tensor routable_count, torch::Tensor extra_zero)
{
    CHECK_DEV(first);
    const int J = (int)first.size(0);
    TORCH_CHECK(out_decision.size(0) >= J && denied_slots.size(0) >= J &&
                allowed_slots.size(0) >= J && states.size(0) >= J &&
                deadlines.size(0) >= J && pick.size(0) >= J &&
                j_poolmask.size(0) >= J && j_labels.size(0) >= J &&
                routable_slots.size(0) >= J && routable_widx.size(0) >= J,
                "per-job tensors must cover J");
    // the spread reads order[j % min(valid_count, K)]
    TORCH_CHECK(K <= order.size(0), "K exceeds the order table");
    const int n_extra = (int)extra_zero.size(0);
    const int blocks = (std::max(std::max(J, n_extra), 1) + BLOCK - 1) / BLOCK;
    hipLaunchKernelGGL(gate_route_kernel, dim3(blocks), dim3(BLOCK), 0, cur_stream(),
        first.data_ptr<int>(), (const signed char*)decisions.data_ptr<int8_t>(),
        (signed char*)out_decision.data_ptr<int8_t>(),
        denied_slots.data_ptr<int>(), denied_count.data_ptr<int>(),
        allowed_slots.data_ptr<int>(), allowed_count.data_ptr<int>(),
        states.data_ptr<uint8_t>(), (long long*)deadlines.data_ptr<int64_t>(),
        dlq_ring.data_ptr<int>(), dlq_head.data_ptr<int>(), (int)dlq_ring.size(0),
        pick.data_ptr<int>(), order.data_ptr<int>(), valid_count.data_ptr<int>(),
        (const long long*)j_poolmask.data_ptr<int64_t>(),
        (const long long*)j_labels.data_ptr<int64_t>(),
        (long long)full_mask, (int)K,
        routable_slots.data_ptr<int>(), routable_widx.data_ptr<int>(),
        routable_count.data_ptr<int>(),
        extra_zero.data_ptr<int>(), n_extra,
        J, (int)decisions.size(0));
}

void tick_finish(torch::Tensor ctx_arena, torch::Tensor routable_slots,
                 torch::Tensor routable_widx, torch::Tensor routable_count,
                 torch::Tensor res_arena, torch::Tensor res_sum, int64_t stride,
                 torch::Tensor states, torch::Tensor attempts, torch::Tensor deadlines,
                 std::vector<int64_t> chain,
                 torch::Tensor w_active_local, int64_t nwl, int64_t my_rank,
                 torch::Tensor counts, torch::Tensor acc, int64_t capacity)
{
    CHECK_DEV(ctx_arena);
    TORCH_CHECK(capacity <= routable_slots.size(0) && capacity <= routable_widx.size(0),
                "capacity exceeds the routable lists");
    TORCH_CHECK(ctx_arena.numel() >= capacity * stride && res_arena.numel() >= capacity * stride &&
                res_sum.size(0) >= capacity && states.size(0) >= capacity,
                "arenas must cover capacity slots");
    TORCH_CHECK(nwl > 0 && w_active_local.size(0) >= nwl, "w_active_local must be [nwl]");
    TORCH_CHECK(acc.size(0) >= counts.size(0) && counts.size(0) <= BLOCK, "acc must cover counts");
    const auto to = unpack_chain(chain);
    const int waves_per_block = BLOCK / WAVE;
    const int blocks = (std::max((int)capacity, 1) + waves_per_block - 1) / waves_per_block;
    hipLaunchKernelGGL(tick_finish_kernel, dim3(blocks), dim3(BLOCK), 0, cur_stream(),
        (const unsigned int*)ctx_arena.data_ptr<int32_t>(),
        routable_slots.data_ptr<int>(), routable_widx.data_ptr<int>(),
        routable_count.data_ptr<int>(),
        (unsigned int*)res_arena.data_ptr<int32_t>(),
        (unsigned int*)res_sum.data_ptr<int32_t>(), (int)stride,
        states.data_ptr<uint8_t>(), attempts.data_ptr<int>(),
        (long long*)deadlines.data_ptr<int64_t>(),
        to[0], to[1], to[2], to[3],
        w_active_local.data_ptr<int>(), (int)nwl, (int)my_rank,
        counts.data_ptr<int>(), (long long*)acc.data_ptr<int64_t>(), (int)counts.size(0));
}

std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor> run_readiness(
    torch::Tensor step_state, torch::Tensor deps_mask, torch::Tensor n_steps,
    torch::Tensor run_active, int64_t cap)
{
    CHECK_DEV(step_state);
    const int NR = (int)step_state.size(0);
    auto opts_i = torch::TensorOptions().dtype(torch::kInt32).device(step_state.device());
    auto ready = torch::zeros({NR}, torch::TensorOptions().dtype(torch::kInt64).device(step_state.device()));
    auto runs = torch::empty({cap}, opts_i);
    auto steps = torch::empty({cap}, opts_i);
    auto count = torch::zeros({1}, opts_i);
    if (NR == 0) return {ready, runs, steps, count};
    const int blocks = (NR + BLOCK - 1) / BLOCK;
    hipLaunchKernelGGL(run_readiness_kernel, dim3(blocks), dim3(BLOCK), 0, cur_stream(),
        step_state.data_ptr<uint8_t>(),
        (const long long*)deps_mask.data_ptr<int64_t>(),
        n_steps.data_ptr<uint8_t>(), run_active.data_ptr<uint8_t>(),
        (long long*)ready.data_ptr<int64_t>(),
        runs.data_ptr<int>(), steps.data_ptr<int>(), count.data_ptr<int>(),
        NR, (int)cap);
    return {ready, runs, steps, count};
}


void pack_by_dest(torch::Tensor routable_slots, torch::Tensor routable_widx,
                  torch::Tensor routable_count, torch::Tensor send_slots,
                  torch::Tensor send_widx, torch::Tensor send_cnt,
                  int64_t nwl, int64_t cap, int64_t capacity,
                  torch::Tensor rq_src, torch::Tensor rq_widx,
                  torch::Tensor rq_attempts, torch::Tensor rq_count,
                  torch::Tensor rq_dead,
                  torch::Tensor dead_src, torch::Tensor dead_count)
{
    const int blocks = ((int)capacity + BLOCK - 1) / BLOCK;
    hipLaunchKernelGGL(pack_by_dest_kernel, dim3(blocks), dim3(BLOCK), 0, cur_stream(),
        routable_slots.data_ptr<int>(), routable_widx.data_ptr<int>(),
        routable_count.data_ptr<int>(), send_slots.data_ptr<int>(),
        send_widx.data_ptr<int>(), send_cnt.data_ptr<int>(), (int)nwl, (int)cap,
        rq_src.data_ptr<int>(), rq_widx.data_ptr<int>(),
        rq_attempts.data_ptr<int>(), rq_count.data_ptr<int>(),
        (unsigned long long*)rq_dead.data_ptr<int64_t>(),
        (int)rq_src.size(0),
        dead_src.data_ptr<int>(), dead_count.data_ptr<int>(),
        (int)dead_src.size(0));
}

void pack_requeue(torch::Tensor rq_prev_widx, torch::Tensor rq_prev_attempts,
                  torch::Tensor rq_prev_count, torch::Tensor send_slots,
                  torch::Tensor send_widx, torch::Tensor send_cnt,
                  int64_t nwl, int64_t cap,
                  torch::Tensor rq_src, torch::Tensor rq_widx,
                  torch::Tensor rq_attempts, torch::Tensor rq_count,
                  torch::Tensor rq_dead,
                  torch::Tensor dead_src, torch::Tensor dead_count)
{
    const int rq_cap = (int)rq_src.size(0);
    const int blocks = (rq_cap + BLOCK - 1) / BLOCK;
    hipLaunchKernelGGL(pack_requeue_kernel, dim3(blocks), dim3(BLOCK), 0, cur_stream(),
        rq_prev_widx.data_ptr<int>(), rq_prev_attempts.data_ptr<int>(),
        rq_prev_count.data_ptr<int>(), send_slots.data_ptr<int>(),
        send_widx.data_ptr<int>(), send_cnt.data_ptr<int>(), (int)nwl, (int)cap,
        rq_src.data_ptr<int>(), rq_widx.data_ptr<int>(),
        rq_attempts.data_ptr<int>(), rq_count.data_ptr<int>(),
        (unsigned long long*)rq_dead.data_ptr<int64_t>(), rq_cap,
        dead_src.data_ptr<int>(), dead_count.data_ptr<int>(),
        (int)dead_src.size(0));
}

void wf_sweep(torch::Tensor step_state, torch::Tensor deps_mask, torch::Tensor n_steps,
              torch::Tensor run_active, torch::Tensor step_kind, torch::Tensor cond_bits,
              torch::Tensor next_ready, torch::Tensor tick,
              torch::Tensor disp_runs, torch::Tensor disp_steps, torch::Tensor disp_count,
              torch::Tensor appr_runs, torch::Tensor appr_steps, torch::Tensor appr_count)
{
    const int NR = (int)n_steps.size(0);
    const int blocks = (NR + BLOCK - 1) / BLOCK;
    hipLaunchKernelGGL(wf_sweep_kernel, dim3(blocks), dim3(BLOCK), 0, cur_stream(),
        step_state.data_ptr<uint8_t>(), (const long long*)deps_mask.data_ptr<int64_t>(),
        n_steps.data_ptr<uint8_t>(), run_active.data_ptr<uint8_t>(),
        step_kind.data_ptr<uint8_t>(), (const long long*)cond_bits.data_ptr<int64_t>(),
        next_ready.data_ptr<int>(), tick.data_ptr<int>(),
        disp_runs.data_ptr<int>(), disp_steps.data_ptr<int>(), disp_count.data_ptr<int>(),
        appr_runs.data_ptr<int>(), appr_steps.data_ptr<int>(), appr_count.data_ptr<int>(),
        NR, (int)disp_runs.size(0), (int)appr_runs.size(0));
}

void wf_expand(torch::Tensor disp_runs, torch::Tensor disp_steps, torch::Tensor disp_count,
               torch::Tensor step_state, torch::Tensor children_todo, torch::Tensor children_out,
               torch::Tensor max_parallel,
               torch::Tensor child_tag, torch::Tensor child_seq, torch::Tensor child_widx,
               torch::Tensor child_count, torch::Tensor children_emitted,
               torch::Tensor dispatch_tick, torch::Tensor tick,
               torch::Tensor order, torch::Tensor valid_count)
{
    const int cap = (int)disp_runs.size(0);
    const int blocks = (cap + (BLOCK / WAVE) - 1) / (BLOCK / WAVE);
    hipLaunchKernelGGL(wf_expand_kernel, dim3(blocks), dim3(BLOCK), 0, cur_stream(),
        disp_runs.data_ptr<int>(), disp_steps.data_ptr<int>(), disp_count.data_ptr<int>(),
        step_state.data_ptr<uint8_t>(), children_todo.data_ptr<int>(),
        children_out.data_ptr<int>(), max_parallel.data_ptr<int>(), child_tag.data_ptr<int>(),
        child_seq.data_ptr<int>(), child_widx.data_ptr<int>(), child_count.data_ptr<int>(),
        children_emitted.data_ptr<int>(),
        dispatch_tick.data_ptr<int>(), tick.data_ptr<int>(),
        order.data_ptr<int>(), valid_count.data_ptr<int>(),
        cap, (int)child_tag.size(0));
}

void wf_timeout_scan(torch::Tensor step_state, torch::Tensor children_out,
                     torch::Tensor children_fail, torch::Tensor dispatch_tick,
                     torch::Tensor tick, int64_t cutoff, torch::Tensor timeout_count)
{
    const int NRS = (int)step_state.numel();
    const int blocks = (NRS + BLOCK - 1) / BLOCK;
    hipLaunchKernelGGL(wf_timeout_scan_kernel, dim3(blocks), dim3(BLOCK), 0, cur_stream(),
        step_state.data_ptr<uint8_t>(), children_out.data_ptr<int>(),
        children_fail.data_ptr<int>(), dispatch_tick.data_ptr<int>(),
        tick.data_ptr<int>(), (int)cutoff,
        (unsigned long long*)timeout_count.data_ptr<int64_t>(), NRS);
}

void wf_readmit(torch::Tensor run_active, torch::Tensor run_state, torch::Tensor n_steps,
                torch::Tensor step_state, torch::Tensor step_attempts,
                torch::Tensor children_todo, torch::Tensor children_out,
                torch::Tensor children_done, torch::Tensor children_fail,
                torch::Tensor children_emitted, torch::Tensor next_ready,
                torch::Tensor dispatch_tick, torch::Tensor todo_tmpl,
                torch::Tensor nready_tmpl, int64_t filter_state,
                torch::Tensor admit_count)
{
    const int NR = (int)n_steps.size(0);
    const int blocks = (NR + BLOCK - 1) / BLOCK;
    hipLaunchKernelGGL(wf_readmit_kernel, dim3(blocks), dim3(BLOCK), 0, cur_stream(),
        run_active.data_ptr<uint8_t>(), run_state.data_ptr<uint8_t>(),
        n_steps.data_ptr<uint8_t>(), step_state.data_ptr<uint8_t>(),
        step_attempts.data_ptr<int>(), children_todo.data_ptr<int>(),
        children_out.data_ptr<int>(), children_done.data_ptr<int>(),
        children_fail.data_ptr<int>(), children_emitted.data_ptr<int>(),
        next_ready.data_ptr<int>(), dispatch_tick.data_ptr<int>(),
        todo_tmpl.data_ptr<int>(), nready_tmpl.data_ptr<int>(),
        (int)filter_state,
        (unsigned long long*)admit_count.data_ptr<int64_t>(), NR);
}

void wf_apply(torch::Tensor send_slots, torch::Tensor send_cnt, torch::Tensor child_tag,
              torch::Tensor child_seq, torch::Tensor rq_prev_tag, torch::Tensor rq_prev_seq,
              torch::Tensor children_done,
              torch::Tensor children_fail, torch::Tensor children_out,
              int64_t fail_ppt, int64_t drop_ppt, int64_t cap, int64_t world)
{
    const int n = (int)(world * cap);
    const int blocks = (n + BLOCK - 1) / BLOCK;
    hipLaunchKernelGGL(wf_apply_kernel, dim3(blocks), dim3(BLOCK), 0, cur_stream(),
        send_slots.data_ptr<int>(), send_cnt.data_ptr<int>(), child_tag.data_ptr<int>(),
        child_seq.data_ptr<int>(), rq_prev_tag.data_ptr<int>(), rq_prev_seq.data_ptr<int>(),
        children_done.data_ptr<int>(),
        children_fail.data_ptr<int>(), children_out.data_ptr<int>(),
        (int)fail_ppt, (int)drop_ppt, (int)cap, (int)world);
}

void wf_apply_dead(torch::Tensor dead_src, torch::Tensor dead_count, torch::Tensor child_tag,
                   torch::Tensor rq_prev_tag, torch::Tensor children_fail,
                   torch::Tensor children_out)
{
    const int dcap = (int)dead_src.size(0);
    const int blocks = (dcap + BLOCK - 1) / BLOCK;
    hipLaunchKernelGGL(wf_apply_dead_kernel, dim3(blocks), dim3(BLOCK), 0, cur_stream(),
        dead_src.data_ptr<int>(), dead_count.data_ptr<int>(), child_tag.data_ptr<int>(),
        rq_prev_tag.data_ptr<int>(), children_fail.data_ptr<int>(),
        children_out.data_ptr<int>(), dcap);
}

void wf_commit(torch::Tensor step_state, torch::Tensor step_attempts,
               torch::Tensor children_todo, torch::Tensor children_out,
               torch::Tensor children_done, torch::Tensor children_fail,
               torch::Tensor max_parallel,
               torch::Tensor next_ready, torch::Tensor tick, int64_t max_retries,
               torch::Tensor retry_count)
{
    const int NRS = (int)step_state.numel();
    const int blocks = (NRS + BLOCK - 1) / BLOCK;
    hipLaunchKernelGGL(wf_commit_kernel, dim3(blocks), dim3(BLOCK), 0, cur_stream(),
        step_state.data_ptr<uint8_t>(), step_attempts.data_ptr<int>(),
        children_todo.data_ptr<int>(), children_out.data_ptr<int>(),
        children_done.data_ptr<int>(), children_fail.data_ptr<int>(),
        max_parallel.data_ptr<int>(),
        next_ready.data_ptr<int>(), tick.data_ptr<int>(), (int)max_retries,
        (unsigned long long*)retry_count.data_ptr<int64_t>(), NRS);
}

void wf_status(torch::Tensor step_state, torch::Tensor n_steps, torch::Tensor run_active,
               torch::Tensor run_state, torch::Tensor counts)
{
    const int NR = (int)n_steps.size(0);
    const int blocks = (NR + BLOCK - 1) / BLOCK;
    hipLaunchKernelGGL(wf_status_kernel, dim3(blocks), dim3(BLOCK), 0, cur_stream(),
        step_state.data_ptr<uint8_t>(), n_steps.data_ptr<uint8_t>(),
        run_active.data_ptr<uint8_t>(), run_state.data_ptr<uint8_t>(),
        (unsigned long long*)counts.data_ptr<int64_t>(), NR);
}

void wf_grant(torch::Tensor grant_runs, torch::Tensor grant_steps, torch::Tensor verdicts,
              int64_t n, torch::Tensor step_state)
{
    if (n <= 0) return;
    const int blocks = ((int)n + BLOCK - 1) / BLOCK;
    hipLaunchKernelGGL(wf_grant_kernel, dim3(blocks), dim3(BLOCK), 0, cur_stream(),
        grant_runs.data_ptr<int>(), grant_steps.data_ptr<int>(),
        verdicts.data_ptr<uint8_t>(), (int)n, step_state.data_ptr<uint8_t>());
}

// three launches on the current stream: free-slot masks + block counts, the
// scan of the counts, then one wave per request. free_mask / blk_scan are
// caller-owned workspaces ([nblk*4] int64, [nblk+1] int32, nblk = ceil(NR/256))
#define WF_ADMIT_TENSORS \
    torch::Tensor req_tmpl, torch::Tensor req_cond, torch::Tensor req_fanout, \
    torch::Tensor tmpl_deps, torch::Tensor tmpl_kind, torch::Tensor tmpl_todo, \
    torch::Tensor tmpl_maxp, torch::Tensor tmpl_delay, torch::Tensor tmpl_nsteps, \
    torch::Tensor step_state, torch::Tensor step_attempts, \
    torch::Tensor deps_mask, torch::Tensor step_kind, \
    torch::Tensor children_todo, torch::Tensor max_parallel, \
    torch::Tensor children_out, torch::Tensor children_done, \
    torch::Tensor children_fail, torch::Tensor children_emitted, \
    torch::Tensor next_ready, torch::Tensor dispatch_tick, \
    torch::Tensor n_steps, torch::Tensor cond_bits, \
    torch::Tensor run_state, torch::Tensor run_active, \
    torch::Tensor run_life, torch::Tensor run_gen, torch::Tensor tick, \
    torch::Tensor free_mask, torch::Tensor blk_scan, \
    torch::Tensor out_slot, torch::Tensor out_gen, torch::Tensor admit_count
#define WF_ADMIT_TENSOR_ARGS \
    req_tmpl, req_cond, req_fanout, tmpl_deps, tmpl_kind, tmpl_todo, tmpl_maxp, \
    tmpl_delay, tmpl_nsteps, step_state, step_attempts, deps_mask, step_kind, \
    children_todo, max_parallel, children_out, children_done, children_fail, \
    children_emitted, next_ready, dispatch_tick, n_steps, cond_bits, run_state, \
    run_active, run_life, run_gen, tick, free_mask, blk_scan, out_slot, out_gen, \
    admit_count
// the kernel arguments both admission kernels take, from the tensors above
#define WF_ADMIT_KERNEL_ARGS \
    req_tmpl.data_ptr<int>(), (const long long*)req_cond.data_ptr<int64_t>(), \
    req_fanout.data_ptr<int>(), n, \
    (const long long*)tmpl_deps.data_ptr<int64_t>(), tmpl_kind.data_ptr<uint8_t>(), \
    tmpl_todo.data_ptr<int>(), tmpl_maxp.data_ptr<int>(), tmpl_delay.data_ptr<int>(), \
    tmpl_nsteps.data_ptr<uint8_t>(), TC, \
    (const unsigned long long*)free_mask.data_ptr<int64_t>(), \
    blk_scan.data_ptr<int>(), nblk, \
    step_state.data_ptr<uint8_t>(), step_attempts.data_ptr<int>(), \
    (long long*)deps_mask.data_ptr<int64_t>(), step_kind.data_ptr<uint8_t>(), \
    children_todo.data_ptr<int>(), max_parallel.data_ptr<int>(), \
    children_out.data_ptr<int>(), children_done.data_ptr<int>(), \
    children_fail.data_ptr<int>(), children_emitted.data_ptr<int>(), \
    next_ready.data_ptr<int>(), dispatch_tick.data_ptr<int>(), \
    n_steps.data_ptr<uint8_t>(), (long long*)cond_bits.data_ptr<int64_t>(), \
    run_state.data_ptr<uint8_t>(), run_active.data_ptr<uint8_t>(), \
    run_life.data_ptr<uint8_t>(), run_gen.data_ptr<int>(), tick.data_ptr<int>(), \
    out_slot.data_ptr<int>(), out_gen.data_ptr<int>(), \
    (unsigned long long*)admit_count.data_ptr<int64_t>(), NR

// the checks and the two snapshot launches of an admission; `keep` and
// `skip` are null for wf_admit. Returns the request count (0: nothing to do).
static int wf_admit_prepare(const char* op, WF_ADMIT_TENSORS,
                            const torch::Tensor* keep, const torch::Tensor* skip)
{
    const int n = (int)req_tmpl.size(0);
    if (n <= 0) return 0;
    const int NR = (int)n_steps.size(0);
    const int nblk = (NR + BLOCK - 1) / BLOCK;
    TORCH_CHECK(req_cond.size(0) >= n && req_fanout.size(0) >= n
                && out_slot.size(0) >= n && out_gen.size(0) >= n
                && (!keep || (keep->size(0) >= n && skip->size(0) >= n)),
                op, ": request/output arrays shorter than the request count");
    TORCH_CHECK(free_mask.numel() >= (int64_t)nblk * (BLOCK / WAVE)
                && blk_scan.numel() >= nblk + 1, op, ": workspace too small");
    wf_check_numel(op, (int64_t)NR * 64, {step_state});
    wf_check_numel(op, NR, {run_life, run_gen});
    const int TC = (int)tmpl_nsteps.size(0);
    TORCH_CHECK(tmpl_deps.numel() == (int64_t)TC * 64, op, ": template sizes disagree");
    if (keep) {
        TORCH_CHECK(keep->scalar_type() == torch::kInt64 && skip->scalar_type() == torch::kInt64,
                    op, ": the keep and skip masks must be int64");
        wf_check_contiguous(op, {*keep, *skip});
    }
    hipLaunchKernelGGL(wf_admit_count_kernel, dim3(nblk), dim3(BLOCK), 0, cur_stream(),
        run_life.data_ptr<uint8_t>(),
        (unsigned long long*)free_mask.data_ptr<int64_t>(), blk_scan.data_ptr<int>(), NR);
    hipLaunchKernelGGL(wf_admit_scan_kernel, dim3(1), dim3(BLOCK), 0, cur_stream(),
        blk_scan.data_ptr<int>(), nblk);
    return n;
}

void wf_admit(WF_ADMIT_TENSORS)
{
    const int n = wf_admit_prepare("wf_admit", WF_ADMIT_TENSOR_ARGS, nullptr, nullptr);
    if (n <= 0) return;
    const int NR = (int)n_steps.size(0), TC = (int)tmpl_nsteps.size(0);
    const int nblk = (NR + BLOCK - 1) / BLOCK;
    const int blocks = (n + (BLOCK / WAVE) - 1) / (BLOCK / WAVE);
    hipLaunchKernelGGL(wf_admit_kernel, dim3(blocks), dim3(BLOCK), 0, cur_stream(),
        WF_ADMIT_KERNEL_ARGS);
}

// wf_admit with kept steps: the same three launches, the last one the kernel
// that validates and presets the steps named by req_keep / req_skip ([n] int64)
void wf_admit_keep(WF_ADMIT_TENSORS, torch::Tensor req_keep, torch::Tensor req_skip)
{
    const int n = wf_admit_prepare("wf_admit_keep", WF_ADMIT_TENSOR_ARGS, &req_keep, &req_skip);
    if (n <= 0) return;
    const int NR = (int)n_steps.size(0), TC = (int)tmpl_nsteps.size(0);
    const int nblk = (NR + BLOCK - 1) / BLOCK;
    const int blocks = (n + (BLOCK / WAVE) - 1) / (BLOCK / WAVE);
    hipLaunchKernelGGL(wf_admit_keep_kernel, dim3(blocks), dim3(BLOCK), 0, cur_stream(),
        WF_ADMIT_KERNEL_ARGS,
        (const long long*)req_keep.data_ptr<int64_t>(),
        (const long long*)req_skip.data_ptr<int64_t>());
}

void wf_cancel(torch::Tensor req_slot, torch::Tensor req_gen,
               torch::Tensor run_life, torch::Tensor run_gen,
               torch::Tensor run_active, torch::Tensor run_state,
               torch::Tensor n_steps, torch::Tensor step_state,
               torch::Tensor cancel_count, torch::Tensor out_ok)
{
    const int n = (int)req_slot.size(0);
    if (n <= 0) return;
    const int NR = (int)n_steps.size(0);
    TORCH_CHECK(req_gen.size(0) >= n && out_ok.size(0) >= n,
                "wf_cancel: request/output arrays shorter than the request count");
    wf_check_numel("wf_cancel", (int64_t)NR * 64, {step_state});
    wf_check_numel("wf_cancel", NR, {run_life, run_gen});
    const int blocks = (n + (BLOCK / WAVE) - 1) / (BLOCK / WAVE);
    hipLaunchKernelGGL(wf_cancel_kernel, dim3(blocks), dim3(BLOCK), 0, cur_stream(),
        req_slot.data_ptr<int>(), req_gen.data_ptr<int>(), n,
        run_life.data_ptr<uint8_t>(), run_gen.data_ptr<int>(),
        run_active.data_ptr<uint8_t>(), run_state.data_ptr<uint8_t>(),
        n_steps.data_ptr<uint8_t>(), step_state.data_ptr<uint8_t>(),
        (unsigned long long*)cancel_count.data_ptr<int64_t>(),
        out_ok.data_ptr<uint8_t>(), NR);
}

void wf_retire(torch::Tensor run_life, torch::Tensor run_active, torch::Tensor run_state,
               torch::Tensor run_gen, torch::Tensor n_steps,
               torch::Tensor children_out, torch::Tensor dispatch_tick,
               torch::Tensor tick, int64_t cutoff,
               torch::Tensor done_slot, torch::Tensor done_gen,
               torch::Tensor done_state, torch::Tensor done_count)
{
    const int NR = (int)n_steps.size(0);
    const int cap = (int)done_slot.size(0);
    TORCH_CHECK(done_gen.size(0) >= cap && done_state.size(0) >= cap,
                "wf_retire: done arrays disagree");
    wf_check_numel("wf_retire", (int64_t)NR * 64, {children_out, dispatch_tick});
    wf_check_numel("wf_retire", NR, {run_life});
    const int blocks = (NR + BLOCK - 1) / BLOCK;
    hipLaunchKernelGGL(wf_retire_kernel, dim3(blocks), dim3(BLOCK), 0, cur_stream(),
        run_life.data_ptr<uint8_t>(), run_active.data_ptr<uint8_t>(),
        run_state.data_ptr<uint8_t>(), run_gen.data_ptr<int>(),
        n_steps.data_ptr<uint8_t>(), children_out.data_ptr<int>(),
        dispatch_tick.data_ptr<int>(), tick.data_ptr<int>(), (int)cutoff,
        done_slot.data_ptr<int>(), done_gen.data_ptr<int>(),
        done_state.data_ptr<int>(), done_count.data_ptr<int>(), NR, cap);
}

// one journal pass on the current stream; cap is ev_rec's length in records
void wf_journal(torch::Tensor step_state, torch::Tensor run_life, torch::Tensor run_gen,
                torch::Tensor tick, int64_t phase,
                torch::Tensor ev_shadow_state, torch::Tensor ev_shadow_gen,
                torch::Tensor ev_rec, torch::Tensor ev_count)
{
    const int64_t NR = run_life.numel();
    const int64_t cap = ev_rec.numel() / 4;
    if (NR <= 0) return;
    wf_check_numel("wf_journal", NR * 64, {step_state, ev_shadow_state});
    wf_check_numel("wf_journal", NR, {run_gen, ev_shadow_gen});
    TORCH_CHECK(cap >= 1 && ev_rec.numel() == cap * 4 && ev_count.numel() >= 1
                && tick.numel() >= 1, "wf_journal: event list needs cap*4 words, cap >= 1");
    wf_check_contiguous("wf_journal", {step_state, ev_shadow_state, ev_rec});
    // the counter's bound (see the kernel) and the 4-lanes-per-row grid in int
    TORCH_CHECK(cap + 64 * NR + 1024 <= (int64_t)INT_MAX,
                "wf_journal: cap + 64*NR would let the event counter wrap");
    wf_check_aligned16("wf_journal", "states, shadow and records",
                       {step_state, ev_shadow_state, ev_rec});
    hipLaunchKernelGGL(wf_journal_kernel, dim3(wf_row_grid(NR)), dim3(BLOCK), 0, cur_stream(),
        step_state.data_ptr<uint8_t>(), run_life.data_ptr<uint8_t>(),
        run_gen.data_ptr<int>(), tick.data_ptr<int>(), (int)phase,
        ev_shadow_state.data_ptr<uint8_t>(), ev_shadow_gen.data_ptr<int>(),
        ev_rec.data_ptr<int>(), ev_count.data_ptr<int>(), (int)NR, (int)cap);
}

// one hold scan on the current stream (inside the tick, after wf_sweep); the
// caller zeroes hold_open first
void wf_hold_scan(torch::Tensor step_state, torch::Tensor n_steps, torch::Tensor run_life,
                  torch::Tensor run_active, torch::Tensor run_gen, torch::Tensor tick,
                  torch::Tensor hold_ttl, torch::Tensor hold_mask, torch::Tensor hold_tick,
                  torch::Tensor hold_gen, torch::Tensor hold_counts, torch::Tensor hold_open)
{
    const int64_t NR = run_life.numel();
    if (NR <= 0) return;
    wf_check_numel("wf_hold_scan", NR * 64, {step_state, hold_ttl, hold_tick});
    wf_check_numel("wf_hold_scan", NR, {n_steps, run_active, run_gen, hold_mask, hold_gen});
    TORCH_CHECK(hold_counts.numel() >= 4 && hold_open.numel() >= 1 && tick.numel() >= 1,
                "wf_hold_scan: counters need 4 + 1 words");
    wf_check_contiguous("wf_hold_scan", {step_state, hold_ttl, hold_tick, hold_mask});
    wf_check_fits_int("wf_hold_scan", NR * 64 + 1024);
    wf_check_aligned16("wf_hold_scan", "states", {step_state});
    hipLaunchKernelGGL(wf_hold_scan_kernel, dim3(wf_row_grid(NR)), dim3(BLOCK), 0, cur_stream(),
        step_state.data_ptr<uint8_t>(), n_steps.data_ptr<uint8_t>(),
        run_life.data_ptr<uint8_t>(), run_active.data_ptr<uint8_t>(),
        run_gen.data_ptr<int>(), tick.data_ptr<int>(), hold_ttl.data_ptr<int>(),
        (unsigned long long*)hold_mask.data_ptr<int64_t>(), hold_tick.data_ptr<int>(),
        hold_gen.data_ptr<int>(), (unsigned long long*)hold_counts.data_ptr<int64_t>(),
        hold_open.data_ptr<int>(), (int)NR);
}

// one settle pass on the current stream (inside the tick, in place of
// wf_timeout_scan + wf_commit); tmpl_policy is [TC*64*4], tmpl_timeout [TC*64]
void wf_settle(torch::Tensor step_state, torch::Tensor step_attempts,
               torch::Tensor children_todo, torch::Tensor children_out,
               torch::Tensor children_fail, torch::Tensor max_parallel,
               torch::Tensor next_ready, torch::Tensor dispatch_tick,
               torch::Tensor run_life, torch::Tensor run_tmpl,
               torch::Tensor tmpl_policy, torch::Tensor tmpl_timeout,
               torch::Tensor tick, torch::Tensor timeout_count, torch::Tensor retry_count)
{
    const int64_t NR = run_life.numel();
    const int64_t TC = tmpl_timeout.numel() / 64;
    if (NR <= 0) return;
    wf_check_numel("wf_settle", NR * 64,
                   {step_state, step_attempts, children_todo, children_out, children_fail,
                    max_parallel, next_ready, dispatch_tick});
    wf_check_numel("wf_settle", NR, {run_tmpl});
    TORCH_CHECK(TC >= 1 && tmpl_timeout.numel() == TC * 64
                && tmpl_policy.numel() == TC * 64 * 4 && TC * 64 <= (int64_t)INT_MAX,
                "wf_settle: policy tables need TC*64*4 and TC*64 words, TC >= 1");
    TORCH_CHECK(tick.numel() >= 1 && timeout_count.numel() >= 1 && retry_count.numel() >= 1,
                "wf_settle: tick and counters need one word each");
    wf_check_contiguous("wf_settle",
                        {step_state, step_attempts, children_todo, children_out, children_fail,
                         max_parallel, next_ready, dispatch_tick, run_tmpl, tmpl_policy,
                         tmpl_timeout});
    wf_check_fits_int("wf_settle", NR * 64 + 1024);
    wf_check_aligned16("wf_settle", "states and policy records", {step_state, tmpl_policy});
    hipLaunchKernelGGL(wf_settle_kernel, dim3(wf_row_grid(NR)), dim3(BLOCK), 0, cur_stream(),
        step_state.data_ptr<uint8_t>(), step_attempts.data_ptr<int>(),
        children_todo.data_ptr<int>(), children_out.data_ptr<int>(),
        children_fail.data_ptr<int>(), max_parallel.data_ptr<int>(),
        next_ready.data_ptr<int>(), dispatch_tick.data_ptr<int>(),
        run_life.data_ptr<uint8_t>(), run_tmpl.data_ptr<int>(),
        reinterpret_cast<const int4*>(tmpl_policy.data_ptr<int>()),
        tmpl_timeout.data_ptr<int>(), tick.data_ptr<int>(),
        (unsigned long long*)timeout_count.data_ptr<int64_t>(),
        (unsigned long long*)retry_count.data_ptr<int64_t>(), (int)NR, (int)TC);
}

// one predicate pass on the current stream (inside the tick, directly before
// wf_sweep); tmpl_cond is [TC*64*4], tmpl_cond_mask [TC], run_input [NR*IW]
void wf_cond_eval(torch::Tensor step_state, torch::Tensor deps_mask, torch::Tensor step_kind,
                  torch::Tensor run_life, torch::Tensor run_active, torch::Tensor run_tmpl,
                  torch::Tensor tmpl_cond, torch::Tensor tmpl_cond_mask,
                  torch::Tensor run_input, torch::Tensor step_out, torch::Tensor cond_bits,
                  torch::Tensor cond_counts, int64_t input_words)
{
    const int64_t NR = run_life.numel();
    const int64_t TC = tmpl_cond_mask.numel();
    const int64_t IW = input_words;
    if (NR <= 0) return;
    wf_check_numel("wf_cond_eval", NR * 64, {step_state, deps_mask, step_kind, step_out});
    wf_check_numel("wf_cond_eval", NR, {run_active, run_tmpl, cond_bits});
    TORCH_CHECK(IW >= 1 && IW <= 32 && run_input.numel() == NR * IW,
                "wf_cond_eval: run_input needs NR*input_words words, 1 <= input_words <= 32");
    TORCH_CHECK(TC >= 1 && tmpl_cond.numel() == TC * 64 * 4 && TC * 64 <= (int64_t)INT_MAX,
                "wf_cond_eval: predicate tables need TC*64*4 and TC words, TC >= 1");
    TORCH_CHECK(cond_counts.numel() >= 2, "wf_cond_eval: counters need two words");
    wf_check_contiguous("wf_cond_eval",
                        {step_state, deps_mask, step_kind, run_life, run_active, run_tmpl,
                         tmpl_cond, tmpl_cond_mask, run_input, step_out, cond_bits});
    wf_check_fits_int("wf_cond_eval", NR * 64 + 1024);
    wf_check_aligned16("wf_cond_eval", "states and predicate records", {step_state, tmpl_cond});
    hipLaunchKernelGGL(wf_cond_eval_kernel, dim3(wf_row_grid(NR)), dim3(BLOCK), 0, cur_stream(),
        step_state.data_ptr<uint8_t>(), (const long long*)deps_mask.data_ptr<int64_t>(),
        step_kind.data_ptr<uint8_t>(), run_life.data_ptr<uint8_t>(),
        run_active.data_ptr<uint8_t>(), run_tmpl.data_ptr<int>(),
        reinterpret_cast<const int4*>(tmpl_cond.data_ptr<int>()),
        (const unsigned long long*)tmpl_cond_mask.data_ptr<int64_t>(),
        run_input.data_ptr<int>(), step_out.data_ptr<int>(),
        (unsigned long long*)cond_bits.data_ptr<int64_t>(),
        (unsigned long long*)cond_counts.data_ptr<int64_t>(), (int)NR, (int)TC, (int)IW);
}

// payload rows of the children emitted this tick (after wf_expand); the grid
// is fixed, the count is read on the device
void wf_child_payload(torch::Tensor child_tag, torch::Tensor child_seq,
                      torch::Tensor child_count, torch::Tensor run_input,
                      torch::Tensor child_payload, int64_t input_words, int64_t payload_words)
{
    const int64_t CB = child_tag.numel();
    const int64_t IW = input_words, W = payload_words;
    if (CB <= 0) return;
    TORCH_CHECK(IW >= 1 && IW <= 32 && W >= IW + 2,
                "wf_child_payload: needs 1 <= input_words <= 32, payload_words >= input_words + 2");
    TORCH_CHECK(child_seq.numel() == CB && child_count.numel() >= 1
                && child_payload.numel() == CB * W && run_input.numel() % IW == 0
                && run_input.numel() >= IW, "wf_child_payload: table sizes disagree");
    TORCH_CHECK(CB * W <= (int64_t)INT_MAX && run_input.numel() <= (int64_t)INT_MAX,
                "wf_child_payload: arena too large");
    wf_check_contiguous("wf_child_payload", {child_tag, child_seq, run_input, child_payload});
    const int64_t NR = run_input.numel() / IW;
    // 4 rows per block and pass; 2048 blocks fill the device at 8 waves/SIMD
    const int blocks = (int)std::min<int64_t>((CB + BLOCK / WAVE - 1) / (BLOCK / WAVE), 2048);
    hipLaunchKernelGGL(wf_child_payload_kernel, dim3(blocks), dim3(BLOCK), 0, cur_stream(),
        child_tag.data_ptr<int>(), child_seq.data_ptr<int>(), child_count.data_ptr<int>(),
        run_input.data_ptr<int>(), child_payload.data_ptr<int>(),
        (int)CB, (int)NR, (int)IW, (int)W);
}

// wf_apply plus the step outputs: sums_back is [world*cap], step_out [NR*64]
void wf_apply_out(torch::Tensor send_slots, torch::Tensor send_cnt, torch::Tensor child_tag,
                  torch::Tensor child_seq, torch::Tensor rq_prev_tag, torch::Tensor rq_prev_seq,
                  torch::Tensor children_done,
                  torch::Tensor children_fail, torch::Tensor children_out,
                  torch::Tensor sums_back, torch::Tensor step_out,
                  int64_t fail_ppt, int64_t drop_ppt, int64_t cap, int64_t world)
{
    const int n = (int)(world * cap);
    TORCH_CHECK(send_slots.numel() >= n && sums_back.numel() >= n && send_cnt.numel() >= world,
                "wf_apply_out: send tables need world*cap entries");
    wf_check_numel("wf_apply_out", children_done.numel(),
                   {step_out, children_fail, children_out});
    wf_check_contiguous("wf_apply_out", {sums_back, step_out});
    const int blocks = (n + BLOCK - 1) / BLOCK;
    hipLaunchKernelGGL(wf_apply_out_kernel, dim3(blocks), dim3(BLOCK), 0, cur_stream(),
        send_slots.data_ptr<int>(), send_cnt.data_ptr<int>(), child_tag.data_ptr<int>(),
        child_seq.data_ptr<int>(), rq_prev_tag.data_ptr<int>(), rq_prev_seq.data_ptr<int>(),
        children_done.data_ptr<int>(),
        children_fail.data_ptr<int>(), children_out.data_ptr<int>(),
        (const unsigned int*)sums_back.data_ptr<int>(), (unsigned int*)step_out.data_ptr<int>(),
        (int)fail_ppt, (int)drop_ppt, (int)cap, (int)world);
}

// one page of open holds, three launches on the current stream. list is
// [count, pad x3 | cap records of 4 words]; list_mask / blk_scan are
// caller-owned workspaces ([NR] int64, [nblk+1] int32, nblk = ceil(NR/256))
void wf_hold_list(torch::Tensor step_state, torch::Tensor run_life, torch::Tensor run_active,
                  torch::Tensor run_gen, torch::Tensor hold_mask, torch::Tensor hold_tick,
                  torch::Tensor hold_gen, int64_t cursor,
                  torch::Tensor list_mask, torch::Tensor blk_scan, torch::Tensor list)
{
    const int64_t NR = run_life.numel();
    if (NR <= 0) return;
    const int nblk = (int)((NR + BLOCK - 1) / BLOCK);
    const int64_t cap = (list.numel() - 4) / 4;
    wf_check_numel("wf_hold_list", NR * 64, {step_state, hold_tick});
    wf_check_numel("wf_hold_list", NR, {run_active, run_gen, hold_mask, hold_gen});
    TORCH_CHECK(list_mask.numel() >= NR && blk_scan.numel() >= nblk + 1,
                "wf_hold_list: workspace too small");
    TORCH_CHECK(cap >= 1 && list.numel() == 4 + cap * 4 && cap <= (int64_t)INT_MAX,
                "wf_hold_list: the list needs 4 + cap*4 words, cap >= 1");
    wf_check_contiguous("wf_hold_list", {step_state, list, hold_tick});
    wf_check_fits_int("wf_hold_list", NR * 64);     // one thread per row: no overshoot
    wf_check_aligned16("wf_hold_list", "states and list", {step_state, list});
    hipLaunchKernelGGL(wf_hold_list_count_kernel, dim3(nblk), dim3(BLOCK), 0, cur_stream(),
        step_state.data_ptr<uint8_t>(), run_life.data_ptr<uint8_t>(),
        run_active.data_ptr<uint8_t>(), run_gen.data_ptr<int>(),
        (const unsigned long long*)hold_mask.data_ptr<int64_t>(), hold_gen.data_ptr<int>(),
        (long long)cursor, (unsigned long long*)list_mask.data_ptr<int64_t>(),
        blk_scan.data_ptr<int>(), (int)NR);
    hipLaunchKernelGGL(wf_admit_scan_kernel, dim3(1), dim3(BLOCK), 0, cur_stream(),
        blk_scan.data_ptr<int>(), nblk);
    hipLaunchKernelGGL(wf_hold_list_write_kernel, dim3(nblk), dim3(BLOCK), 0, cur_stream(),
        (const unsigned long long*)list_mask.data_ptr<int64_t>(), blk_scan.data_ptr<int>(),
        run_gen.data_ptr<int>(), hold_tick.data_ptr<int>(), list.data_ptr<int>(),
        (int)NR, nblk, (int)cap);
}

void wf_decide(torch::Tensor req_slot, torch::Tensor req_gen, torch::Tensor req_step,
               torch::Tensor req_verdict,
               torch::Tensor run_life, torch::Tensor run_gen, torch::Tensor run_active,
               torch::Tensor n_steps, torch::Tensor step_kind, torch::Tensor step_state,
               torch::Tensor hold_counts, torch::Tensor out_code)
{
    const int n = (int)req_slot.size(0);
    if (n <= 0) return;
    const int64_t NR = n_steps.size(0);
    TORCH_CHECK(req_gen.size(0) >= n && req_step.size(0) >= n && req_verdict.size(0) >= n
                && out_code.size(0) >= n,
                "wf_decide: request/output arrays shorter than the request count");
    wf_check_numel("wf_decide", NR * 64, {step_state, step_kind});
    wf_check_numel("wf_decide", NR, {run_life, run_gen, run_active});
    TORCH_CHECK(hold_counts.numel() >= 4, "wf_decide: table sizes disagree");
    const int blocks = (n + BLOCK - 1) / BLOCK;
    hipLaunchKernelGGL(wf_decide_kernel, dim3(blocks), dim3(BLOCK), 0, cur_stream(),
        req_slot.data_ptr<int>(), req_gen.data_ptr<int>(), req_step.data_ptr<int>(),
        req_verdict.data_ptr<int>(), n,
        run_life.data_ptr<uint8_t>(), run_gen.data_ptr<int>(),
        run_active.data_ptr<uint8_t>(), n_steps.data_ptr<uint8_t>(),
        step_kind.data_ptr<uint8_t>(), step_state.data_ptr<uint8_t>(),
        (unsigned long long*)hold_counts.data_ptr<int64_t>(),
        out_code.data_ptr<uint8_t>(), (int)NR);
}

void materialize_rq_payload(torch::Tensor payload, torch::Tensor rq_prev_payload,
                            torch::Tensor rq_src, torch::Tensor rq_count,
                            torch::Tensor rq_payload, int64_t stride)
{
    const int rq_cap = (int)rq_src.size(0);
    const int blocks = (rq_cap + (BLOCK / WAVE) - 1) / (BLOCK / WAVE);
    hipLaunchKernelGGL(materialize_rq_payload_kernel, dim3(blocks), dim3(BLOCK), 0, cur_stream(),
        (const unsigned int*)payload.data_ptr<int32_t>(),
        (const unsigned int*)rq_prev_payload.data_ptr<int32_t>(),
        rq_src.data_ptr<int>(), rq_count.data_ptr<int>(),
        (unsigned int*)rq_payload.data_ptr<int32_t>(), (int)stride, rq_cap);
}

void gather_payload_padded(torch::Tensor payload, torch::Tensor rq_prev_payload,
                           torch::Tensor send_slots,
                           torch::Tensor send_cnt, torch::Tensor send_payload,
                           int64_t stride, int64_t cap, int64_t world)
{
    const int waves = (int)(world * cap);
    const int blocks = (waves + (BLOCK / WAVE) - 1) / (BLOCK / WAVE);
    hipLaunchKernelGGL(gather_payload_padded_kernel, dim3(blocks), dim3(BLOCK), 0, cur_stream(),
        (const unsigned int*)payload.data_ptr<int32_t>(),
        (const unsigned int*)rq_prev_payload.data_ptr<int32_t>(),
        send_slots.data_ptr<int>(),
        send_cnt.data_ptr<int>(), (unsigned int*)send_payload.data_ptr<int32_t>(),
        (int)stride, (int)cap, (int)world);
}

void echo_padded(torch::Tensor recv_payload, torch::Tensor recv_cnt,
                 torch::Tensor res_arena, torch::Tensor res_sums,
                 int64_t stride, int64_t cap, int64_t world)
{
    const int waves = (int)(world * cap);
    const int blocks = (waves + (BLOCK / WAVE) - 1) / (BLOCK / WAVE);
    hipLaunchKernelGGL(echo_padded_kernel, dim3(blocks), dim3(BLOCK), 0, cur_stream(),
        (const unsigned int*)recv_payload.data_ptr<int32_t>(), recv_cnt.data_ptr<int>(),
        (unsigned int*)res_arena.data_ptr<int32_t>(),
        (unsigned int*)res_sums.data_ptr<int32_t>(), (int)stride, (int)cap, (int)world);
}

void apply_transitions_padded(torch::Tensor states, torch::Tensor attempts,
                              torch::Tensor deadlines, torch::Tensor slots_pad,
                              torch::Tensor cnt, int64_t to_state, int64_t cap, int64_t world)
{
    const int n = (int)(world * cap);
    const int blocks = (n + BLOCK - 1) / BLOCK;
    hipLaunchKernelGGL(apply_transitions_padded_kernel, dim3(blocks), dim3(BLOCK), 0, cur_stream(),
        states.data_ptr<uint8_t>(), attempts.data_ptr<int>(),
        (long long*)deadlines.data_ptr<int64_t>(), slots_pad.data_ptr<int>(),
        cnt.data_ptr<int>(), (unsigned char)to_state, (int)cap, (int)world);
}

void load_feedback_padded(torch::Tensor recv_widx, torch::Tensor recv_cnt,
                          torch::Tensor w_active_local, int64_t cap, int64_t world)
{
    const int n = (int)(world * cap);
    const int blocks = (n + BLOCK - 1) / BLOCK;
    hipLaunchKernelGGL(load_feedback_padded_kernel, dim3(blocks), dim3(BLOCK), 0, cur_stream(),
        recv_widx.data_ptr<int>(), recv_cnt.data_ptr<int>(),
        w_active_local.data_ptr<int>(), (int)cap, (int)world);
}


// ---------------------------------------------------------------------------
// Host-side fused synthetic-batch encoder (the e2e ingest stand-in).
// The torch-op version (SyntheticEncoder.fresh) is RNG+gather bound at
// ~1 ms/16k batch; this fused pass (counter-based splitmix64 RNG + LUT row
// gather) does the same work at memory speed. It runs SERIAL and releases
// the GIL: the e2e loop overlaps 2-3 encoder threads, each a fully
// independent call — a shared at::parallel_for pool serialized those calls
// (and holding the GIL stalled the submit loop for the whole encode).
// Index draws use Lemire multiply-shift reduction ((u32)h * V >> 32) —
// a plain `% V` was ~half the per-job cost.
// Deterministic: draws depend only on (seed, step, job, stream), so every
// backend and every re-run produces identical batches.
// ---------------------------------------------------------------------------
static inline uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

void synthetic_fresh(torch::Tensor any_bits,   // [B,7,W] int64 (host)
                     torch::Tensor all_bits,   // [B,2,W] int64 (host)
                     torch::Tensor tenant_lut, // [V,W] int64
                     torch::Tensor topic_lut,  // [V,W]
                     torch::Tensor risk_lut,   // [V,W]
                     torch::Tensor req_lut,    // [V,W]
                     int64_t seed, int64_t step,
                     int64_t dim_tenant, int64_t dim_topic, int64_t dim_risk,
                     int64_t all_requires)
{
    TORCH_CHECK(!any_bits.is_cuda(), "synthetic_fresh is a host encoder");
    const int64_t B = any_bits.size(0);
    const int64_t W = any_bits.size(2);
    const int64_t V = tenant_lut.size(0);
    int64_t* any = any_bits.data_ptr<int64_t>();
    int64_t* all = all_bits.data_ptr<int64_t>();
    const int64_t* tl = tenant_lut.data_ptr<int64_t>();
    const int64_t* ol = topic_lut.data_ptr<int64_t>();
    const int64_t* rl = risk_lut.data_ptr<int64_t>();
    const int64_t* ql = req_lut.data_ptr<int64_t>();
    const uint64_t base = splitmix64((uint64_t)seed * 0x5851F42D4C957F2Dull
                                     ^ (uint64_t)step);
    const uint64_t v = (uint64_t)V;
    constexpr uint32_t RISK_CUT = 1288490189u;  // 0.30 * 2^32
    constexpr uint32_t REQ_CUT = 429496730u;    // 0.10 * 2^32
    if (W == 1) {
        // fast path for the e2e bench shape (single bitset word per dim)
        for (int64_t i = 0; i < B; ++i) {
            const uint64_t h0 = splitmix64(base ^ (uint64_t)i);
            const uint64_t h1 = splitmix64(h0);
            const uint64_t h2 = splitmix64(h1);
            const uint64_t t_idx = ((h0 & 0xffffffffull) * v) >> 32;
            const uint64_t o_idx = ((h0 >> 32) * v) >> 32;
            const uint64_t r_idx = ((h1 & 0xffffffffull) * v) >> 32;
            const uint64_t q_idx = ((h1 >> 32) * v) >> 32;
            const bool has_risk = (uint32_t)h2 < RISK_CUT;
            const bool has_req = (uint32_t)(h2 >> 32) < REQ_CUT;
            int64_t* arow = any + (size_t)i * 7;
            arow[dim_tenant] = tl[t_idx];
            arow[dim_topic] = ol[o_idx];
            arow[dim_risk] = has_risk ? rl[r_idx] : 0;
            all[(size_t)i * 2 + all_requires] = has_req ? ql[q_idx] : 0;
        }
        return;
    }
    for (int64_t i = 0; i < B; ++i) {
        const uint64_t h0 = splitmix64(base ^ (uint64_t)i);
        const uint64_t h1 = splitmix64(h0);
        const uint64_t h2 = splitmix64(h1);
        const int64_t t_idx = (int64_t)(((h0 & 0xffffffffull) * v) >> 32);
        const int64_t o_idx = (int64_t)(((h0 >> 32) * v) >> 32);
        const int64_t r_idx = (int64_t)(((h1 & 0xffffffffull) * v) >> 32);
        const int64_t q_idx = (int64_t)(((h1 >> 32) * v) >> 32);
        const bool has_risk = (uint32_t)h2 < RISK_CUT;
        const bool has_req = (uint32_t)(h2 >> 32) < REQ_CUT;
        int64_t* arow = any + (size_t)i * 7 * W;
        int64_t* lrow = all + (size_t)i * 2 * W;
        for (int64_t w = 0; w < W; ++w) {
            arow[dim_tenant * W + w] = tl[t_idx * W + w];
            arow[dim_topic * W + w] = ol[o_idx * W + w];
            arow[dim_risk * W + w] = has_risk ? rl[r_idx * W + w] : 0;
            lrow[all_requires * W + w] = has_req ? ql[q_idx * W + w] : 0;
        }
    }
}

// Whole host-side batch preparation in one GIL-free call: the four synthetic
// dims exactly as synthetic_fresh draws them (synthetic_fresh stays the
// oracle) plus the per-step stamp of payload word 0. The loop lives in
// synthetic_encode.h (blocked hash, runtime-picked ISA, optional 2-way split
// over a thread the call owns).
void synthetic_fresh_stamped(torch::Tensor any_bits,   // [B,7,W] int64 (host)
                             torch::Tensor all_bits,   // [B,2,W] int64 (host)
                             torch::Tensor tenant_lut, torch::Tensor topic_lut,
                             torch::Tensor risk_lut, torch::Tensor req_lut,
                             int64_t seed, int64_t step,
                             int64_t dim_tenant, int64_t dim_topic, int64_t dim_risk,
                             int64_t all_requires,
                             c10::optional<torch::Tensor> payload,  // [B*words] int32 (host)
                             int64_t payload_words,
                             int64_t threads, int64_t isa_cap)
{
    TORCH_CHECK(!any_bits.is_cuda() && !all_bits.is_cuda(),
                "synthetic_fresh_stamped is a host encoder");
    CHECK_CONTIG(any_bits); CHECK_CONTIG(all_bits);
    CHECK_CONTIG(tenant_lut); CHECK_CONTIG(topic_lut);
    CHECK_CONTIG(risk_lut); CHECK_CONTIG(req_lut);
    cordum_enc::EncodeJob a;
    a.B = any_bits.size(0);
    a.W = any_bits.size(2);
    a.V = tenant_lut.size(0);
    TORCH_CHECK(any_bits.size(1) == 7 && all_bits.size(0) == a.B &&
                all_bits.size(1) == 2 && all_bits.size(2) == a.W, "bad batch shape");
    for (const torch::Tensor* l : {&tenant_lut, &topic_lut, &risk_lut, &req_lut})
        TORCH_CHECK(l->size(0) == a.V && l->size(1) == a.W, "bad LUT shape");
    TORCH_CHECK(dim_tenant >= 0 && dim_tenant < 7 && dim_topic >= 0 && dim_topic < 7 &&
                dim_risk >= 0 && dim_risk < 7 && all_requires >= 0 && all_requires < 2,
                "dim index out of range");
    a.any = any_bits.data_ptr<int64_t>();
    a.all = all_bits.data_ptr<int64_t>();
    a.tenant_lut = tenant_lut.data_ptr<int64_t>();
    a.topic_lut = topic_lut.data_ptr<int64_t>();
    a.risk_lut = risk_lut.data_ptr<int64_t>();
    a.req_lut = req_lut.data_ptr<int64_t>();
    a.seed = (uint64_t)seed;
    a.step = (uint64_t)step;
    a.dim_tenant = (int)dim_tenant;
    a.dim_topic = (int)dim_topic;
    a.dim_risk = (int)dim_risk;
    a.all_requires = (int)all_requires;
    a.payload = nullptr;
    a.payload_words = payload_words;
    if (payload.has_value()) {
        TORCH_CHECK(!payload->is_cuda() && payload->is_contiguous() &&
                    payload->scalar_type() == torch::kInt32 && payload_words > 0 &&
                    payload->numel() >= a.B * payload_words, "bad payload ring buffer");
        a.payload = payload->data_ptr<int32_t>();
    }
    cordum_enc::encode_batch(a, (int)threads, (int)isa_cap);
}

// synthetic_fresh_stamped into compact rows: cols [B,L] holds one word per
// dimension the compiled policy reads (ops/policy_mfma.py), col_of_* is the
// column of each synthetic dim or -1 where the policy does not read it. Same
// draws, same stamp; a dim without a column is drawn and not stored. Writes
// nothing else: the other columns and the secrets bytes behind the rows keep
// what the caller put there (zeros, set once at allocation).
void synthetic_fresh_compact(torch::Tensor cols,        // [B,L] int64 (host)
                             torch::Tensor tenant_lut, torch::Tensor topic_lut,
                             torch::Tensor risk_lut, torch::Tensor req_lut,
                             int64_t seed, int64_t step,
                             int64_t col_of_tenant, int64_t col_of_topic,
                             int64_t col_of_risk, int64_t col_of_requires,
                             c10::optional<torch::Tensor> payload,  // [B*words] int32 (host)
                             int64_t payload_words,
                             int64_t threads, int64_t isa_cap)
{
    TORCH_CHECK(!cols.is_cuda(), "synthetic_fresh_compact is a host encoder");
    CHECK_CONTIG(cols);
    CHECK_CONTIG(tenant_lut); CHECK_CONTIG(topic_lut);
    CHECK_CONTIG(risk_lut); CHECK_CONTIG(req_lut);
    TORCH_CHECK(cols.dim() == 2 && cols.scalar_type() == torch::kInt64,
                "cols must be [B,L] int64");
    cordum_enc::EncodeJob a;
    a.B = cols.size(0);
    a.W = 1;
    a.V = tenant_lut.size(0);
    const int64_t L = cols.size(1);
    for (const torch::Tensor* l : {&tenant_lut, &topic_lut, &risk_lut, &req_lut})
        TORCH_CHECK(l->dim() == 2 && l->size(0) == a.V && l->size(1) == 1,
                    "compact rows need 1-word LUTs [V,1]");
    const int64_t c4[4] = {col_of_tenant, col_of_topic, col_of_risk, col_of_requires};
    for (int i = 0; i < 4; ++i) {
        TORCH_CHECK(c4[i] >= -1 && c4[i] < L, "column index out of range");
        for (int k = 0; k < i; ++k)
            TORCH_CHECK(c4[i] < 0 || c4[i] != c4[k], "two dims share a column");
    }
    // both row pointers are the one array; with L == 0 every column is -1
    // and it is never dereferenced
    a.any = a.all = cols.data_ptr<int64_t>();
    a.any_stride = a.all_stride = L;
    a.tenant_lut = tenant_lut.data_ptr<int64_t>();
    a.topic_lut = topic_lut.data_ptr<int64_t>();
    a.risk_lut = risk_lut.data_ptr<int64_t>();
    a.req_lut = req_lut.data_ptr<int64_t>();
    a.seed = (uint64_t)seed;
    a.step = (uint64_t)step;
    a.dim_tenant = (int)col_of_tenant;
    a.dim_topic = (int)col_of_topic;
    a.dim_risk = (int)col_of_risk;
    a.all_requires = (int)col_of_requires;
    a.payload = nullptr;
    a.payload_words = payload_words;
    if (payload.has_value()) {
        TORCH_CHECK(!payload->is_cuda() && payload->is_contiguous() &&
                    payload->scalar_type() == torch::kInt32 && payload_words > 0 &&
                    payload->numel() >= a.B * payload_words, "bad payload ring buffer");
        a.payload = payload->data_ptr<int32_t>();
    }
    cordum_enc::encode_batch(a, (int)threads, (int)isa_cap);
}

void pack_jobs_mfma_dev(torch::Tensor any_bits, torch::Tensor all_bits,
                        torch::Tensor a_pack)
{
    const int B = (int)any_bits.size(0);
    const int Jt = (int)a_pack.size(0);
    const int n = Jt * 9 * 64;
    const int blocks = (n + BLOCK - 1) / BLOCK;
    hipLaunchKernelGGL(pack_jobs_mfma_kernel, dim3(blocks), dim3(BLOCK), 0, cur_stream(),
        (const long long*)any_bits.data_ptr<int64_t>(),
        (const long long*)all_bits.data_ptr<int64_t>(),
        a_pack.data_ptr<int8_t>(), B, Jt);
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    m.def("policy_first_match", &policy_first_match, "K1 batched policy first-match");
    m.def("policy_first_match_mfma", &policy_first_match_mfma, "K1 MFMA comparison variant");
    m.def("worker_precompute", &worker_precompute, "K2a per-worker score/overload precompute");
    m.def("least_loaded_pick", &least_loaded_pick, "K2 least-loaded worker pick");
    m.def("spread_pick", &spread_pick, "K2c batch spreading over the least-loaded set");
    m.def("worker_precompute_into", &worker_precompute_into, "K2a into a persistent key tensor");
    m.def("dlq_ring_append", &dlq_ring_append, "K7 device DLQ ring append");
    m.def("echo_execute_indexed", &echo_execute_indexed, "device echo worker pool (slot-indexed, in-place)");
    m.def("policy_gate", &policy_gate, "decision gather + allow/deny compaction");
    m.def("policy_gate_full", &policy_gate_full,
          "gate + DENIED transition + DLQ ring append in one launch");
    m.def("begin_tick", &begin_tick, "tick prologue: PENDING re-admit + counter reset");
    m.def("accumulate_counts", &accumulate_counts, "fold tick counters into device accumulator");
    m.def("begin_tick_first", &begin_tick_first,
          "tick prologue that also primes the first-match buffer (INT_MAX)");
    m.def("least_loaded_pick_into", &least_loaded_pick_into,
          "K2 pick into a persistent buffer, skipping unconstrained jobs");
    m.def("policy_first_match_mfma_into", &policy_first_match_mfma_into,
          "K1 MFMA into a pre-primed buffer (no alloc/fill launches)");
    m.def("compact_routable_spread", &compact_routable_spread,
          "routable compaction with inline K2c spread");
    m.def("apply_transitions_chain_dyn", &apply_transitions_chain_dyn,
          "K5 chained targets in one launch (+ extra zero region)");
    m.def("compact_routable", &compact_routable, "routable-slot compaction");
    m.def("apply_transitions_dyn", &apply_transitions_dyn, "K5 with device-resident count");
    m.def("echo_execute_indexed_dyn", &echo_execute_indexed_dyn, "echo worker with device count");
    m.def("load_feedback", &load_feedback, "per-worker active-count histogram");
    m.def("run_readiness", &run_readiness, "K3 run/step readiness sweep");
    // GIL released: encoder threads run concurrently with the submit loop
    m.def("synthetic_fresh", &synthetic_fresh,
          py::call_guard<py::gil_scoped_release>(),
          "fused host synthetic-batch encoder");
    m.def("pack_jobs_mfma_dev", &pack_jobs_mfma_dev, "device job packing for the MFMA K1");
    m.def("synthetic_fresh_stamped", &synthetic_fresh_stamped,
          py::call_guard<py::gil_scoped_release>(),
          "host batch preparation in one call: synthetic dims + payload step stamp",
          py::arg("any_bits"), py::arg("all_bits"), py::arg("tenant_lut"),
          py::arg("topic_lut"), py::arg("risk_lut"), py::arg("req_lut"),
          py::arg("seed"), py::arg("step"), py::arg("dim_tenant"), py::arg("dim_topic"),
          py::arg("dim_risk"), py::arg("all_requires"), py::arg("payload"),
          py::arg("payload_words"), py::arg("threads") = 1, py::arg("isa_cap") = -1);
    m.def("synthetic_fresh_compact", &synthetic_fresh_compact,
          py::call_guard<py::gil_scoped_release>(),
          "synthetic_fresh_stamped into compact rows: one column per dim the policy reads",
          py::arg("cols"), py::arg("tenant_lut"), py::arg("topic_lut"),
          py::arg("risk_lut"), py::arg("req_lut"), py::arg("seed"), py::arg("step"),
          py::arg("col_of_tenant"), py::arg("col_of_topic"), py::arg("col_of_risk"),
          py::arg("col_of_requires"), py::arg("payload"), py::arg("payload_words"),
          py::arg("threads") = 1, py::arg("isa_cap") = -1);
    m.def("encoder_isa_level", [] { return cordum_enc::max_isa_level(); },
          "widest encoder ISA this CPU runs (0 baseline, 1 AVX2, 2 AVX-512DQ)");
    m.def("tick_prologue", &tick_prologue,
          "fused tick 1/5: PENDING re-admit + counter reset + first prime + worker keys");
    m.def("policy_first_match_mfma_bits_into", &policy_first_match_mfma_bits_into,
          "fused tick 3/5: K1 MFMA with A fragments built from the staged bit words",
          py::arg("any_bits"), py::arg("all_bits"), py::arg("b_pack"), py::arg("cards"),
          py::arg("rule_secrets"), py::arg("job_secrets"), py::arg("tile_dims"),
          py::arg("n_rules"), py::arg("out"), py::arg("job_tiles") = 1);
    m.def("policy_first_match_mfma_cols_into", &policy_first_match_mfma_cols_into,
          "fused tick 3/5, compact staging: K1 MFMA with A fragments built from the "
          "live-dimension columns",
          py::arg("cols"), py::arg("col_map"), py::arg("b_pack"), py::arg("cards"),
          py::arg("rule_secrets"), py::arg("job_secrets"), py::arg("tile_dims"),
          py::arg("n_rules"), py::arg("out"), py::arg("job_tiles") = 1);
    m.def("gate_route", &gate_route,
          "fused tick 4/5: gate + DENIED/DLQ + spread/exact pick + routable compaction");
    m.def("tick_finish", &tick_finish,
          "fused tick 5/5: echo + state chain + load feedback + counter fold");
    m.def("pack_by_dest", &pack_by_dest, "padded per-destination dispatch pack");
    m.def("pack_requeue", &pack_requeue, "redeliver last tick's requeue ring into the send segments");
    m.def("wf_sweep", &wf_sweep, "K3-WF readiness sweep + approval holds + condition/delay commits");
    m.def("wf_expand", &wf_expand, "K3-WF for_each/worker child expansion into the child arena");
    m.def("wf_apply", &wf_apply, "K3-WF child result application with failure injection");
    m.def("wf_apply_dead", &wf_apply_dead, "K3-WF dead-letter child application");
    m.def("wf_commit", &wf_commit, "K3-WF step aggregation + retry/backoff commit");
    m.def("wf_timeout_scan", &wf_timeout_scan, "K4-WF stale-step timeout scan");
    m.def("wf_readmit", &wf_readmit, "K3-WF continuous run re-admission from template");
    m.def("wf_status", &wf_status, "K3-WF run status roll-up");
    m.def("wf_grant", &wf_grant, "K3-WF host approval grants");
    m.def("wf_admit", &wf_admit, "K3-WF run admission into the lowest free slots");
    m.def("wf_admit_keep", &wf_admit_keep,
          "K3-WF run admission with steps already done (rerun from a step)");
    m.def("wf_cancel", &wf_cancel, "K3-WF generation-checked run cancellation");
    m.def("wf_retire", &wf_retire, "K3-WF completion records + quiescent slot release");
    m.def("wf_journal", &wf_journal, "K3-WF step-transition journal pass (observer)");
    m.def("wf_hold_scan", &wf_hold_scan, "K3-WF approval hold scan (open / expire / close holds)");
    m.def("wf_settle", &wf_settle, "K3-WF per-step-policy timeout + commit pass (replaces the scan/commit pair)");
    m.def("wf_cond_eval", &wf_cond_eval, "K3-WF predicate pass before the sweep (condition bits, guards -> SKIPPED)");
    m.def("wf_child_payload", &wf_child_payload, "K3-WF payload rows of the children emitted this tick");
    m.def("wf_apply_out", &wf_apply_out, "K3-WF child result application with step outputs");
    m.def("wf_hold_list", &wf_hold_list, "K3-WF ordered page of open approval holds");
    m.def("wf_decide", &wf_decide, "K3-WF generation-checked approval decisions");
    m.def("materialize_rq_payload", &materialize_rq_payload, "copy requeued payload rows into the rq arena");
    m.def("gather_payload_padded", &gather_payload_padded, "payload gather into padded send arena");
    m.def("echo_padded", &echo_padded, "region-valid echo over padded recv arena");
    m.def("apply_transitions_padded", &apply_transitions_padded, "K5 over padded slot list");
    m.def("load_feedback_padded", &load_feedback_padded, "padded per-worker load histogram");
    m.def("set_transition_lut", &set_transition_lut, "upload transition legality LUT");
    m.def("apply_transitions", &apply_transitions, "K5 batched state transitions");
    m.def("deadline_scan", &deadline_scan, "K4 deadline/staleness scan");
    m.def("echo_execute", &echo_execute, "device echo worker pool");
}
