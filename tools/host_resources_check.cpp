// Stand-alone check of csrc/host_resources.h (the owners of the host layer's
// device resources and the engine's resource sets), built with the host
// compiler alone and run under the sanitizers by tests/test_cpu_endgame_split.py:
//
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -D__HIP_PLATFORM_AMD__ \
//       -I/opt/rocm/include -I othello-alphazero_amd/csrc tools/host_resources_check.cpp
//
// The HIP entry points the header calls are defined here, over malloc / free:
// they count live objects, log stream and event creations, and can fail the
// k-th creating call. One scenario creates and grows every set; it runs without
// a failure and then once for every creating call, with that call failing:
//   * a call returns an error exactly when a stub failed in it,
//   * after the failed call every set holds what it held before,
//   * the retry succeeds and the run ends in the state of the run without failure,
//   * after destruction nothing is live (a double release: the sanitizer),
//   * streams and events are created in the order the schedules were measured with.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "host_resources.h"

using namespace oamd;

// ---------------------------------------------------------------- the stubs
namespace {
int g_live_dev = 0, g_live_pinned = 0, g_live_events = 0, g_live_streams = 0;
int g_creates = 0;   // creating calls so far
int g_fail_at = 0;   // the creating call that fails (1-based; 0: none)
int g_failed = 0;    // creating calls that failed
std::vector<std::string> g_log;  // "event:<flags>" / "stream:<flags>" per creation
std::string g_err;

bool creating_call_fails() {
    if (++g_creates != g_fail_at) return false;
    ++g_failed;
    return true;
}
}  // namespace

int oamd::fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

extern "C" {
hipError_t hipMalloc(void** p, size_t n) {
    if (creating_call_fails()) return hipErrorOutOfMemory;
    *p = std::malloc(n ? n : 1);
    ++g_live_dev;
    return hipSuccess;
}
hipError_t hipFree(void* p) {
    std::free(p);
    --g_live_dev;
    return hipSuccess;
}
hipError_t hipHostMalloc(void** p, size_t n, unsigned) {
    if (creating_call_fails()) return hipErrorOutOfMemory;
    *p = std::malloc(n ? n : 1);
    ++g_live_pinned;
    return hipSuccess;
}
hipError_t hipHostFree(void* p) {
    std::free(p);
    --g_live_pinned;
    return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned flags) {
    if (creating_call_fails()) return hipErrorOutOfMemory;
    *e = reinterpret_cast<hipEvent_t>(std::malloc(1));
    ++g_live_events;
    g_log.push_back("event:" + std::to_string(flags));
    return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t e) {
    std::free(e);
    --g_live_events;
    return hipSuccess;
}
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned flags) {
    if (creating_call_fails()) return hipErrorOutOfMemory;
    *s = reinterpret_cast<hipStream_t>(std::malloc(1));
    ++g_live_streams;
    g_log.push_back("stream:" + std::to_string(flags));
    return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t s) {
    std::free(s);
    --g_live_streams;
    return hipSuccess;
}
hipError_t hipMemset(void* p, int v, size_t n) {
    std::memset(p, v, n);
    return hipSuccess;
}
hipError_t hipMemcpy(void* d, const void* s, size_t n, hipMemcpyKind) {
    std::memcpy(d, s, n);
    return hipSuccess;
}
hipError_t hipDeviceSynchronize(void) { return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "stub error"; }
hipError_t hipDeviceGetAttribute(int* v, hipDeviceAttribute_t, int) {
    *v = 256;
    return hipSuccess;
}
}

// ---------------------------------------------------------------- the scenario
namespace {

int g_checks = 0, g_failures = 0;
void check(bool ok, const std::string& what) {
    ++g_checks;
    if (!ok) {
        ++g_failures;
        std::printf("FAILED: %s\n", what.c_str());
    }
}

struct Sets {
    RowBuffers rows;
    ReadbackSlots cuts, remaining;
    AdjudicateWorkspace adj;
    SpanWindow spans;
    TimingPools pools;
    PipelineStreams pipe;
    unsigned long long* span = nullptr;  // the last reservation
};

// everything a set holds: pointers, handles, capacities, counts
std::vector<long long> state(const Sets& S) {
    std::vector<long long> v;
    auto p = [&](const void* x) { v.push_back((long long)(intptr_t)x); };
    auto n = [&](long long x) { v.push_back(x); };
    const RowBuffers& r = S.rows;
    for (const void* x : {(const void*)r.leaf.get(), (const void*)r.depth.get(), (const void*)r.trans.get(),
                          (const void*)r.path.get(), (const void*)r.feat.get(), (const void*)r.policy.get(),
                          (const void*)r.value.get(), (const void*)r.flags.get(), (const void*)r.rowlist.get(),
                          (const void*)r.tstate.get()})
        p(x);
    n(r.rows_cap), n(r.fw_cap);
    for (const ReadbackSlots* s : {&S.cuts, &S.remaining}) {
        p(s->dev.get()), p(s->host.get());
        for (auto& row : s->ev)
            for (auto& e : row) p(e.get());
    }
    const AdjudicateWorkspace& a = S.adj;
    p(a.pending.get()), p(a.move_scores.get()), p(a.score.get()), p(a.flags.get()), p(a.solve_ws.get());
    p(a.ev[0].get()), p(a.ev[1].get());
    n(a.pending_cap), n(a.chunk_cap), n(a.solve_ws_bytes), n(a.cus);
    n((long long)S.spans.chunks.size()), n(S.spans.slots), n(S.spans.dropped);
    for (auto& c : S.spans.chunks) p(c.p.get()), n(c.cap), n(c.used);
    for (auto& pool : S.pools.ev) {
        n((long long)pool.size());
        for (auto& e : pool) p(e.get());
    }
    const PipelineStreams& q = S.pipe;
    n(q.n_streams), n(q.n_events), p(q.fork_ev.get()), p(q.idle.get());
    for (auto& e : q.nn_token) p(e.get());
    for (int k = 0; k < kMaxPipeline; ++k) p(q.stream[k].get()), p(q.join_ev[k].get()), p(q.sel_ev[k].get());
    return v;
}

// the same without the addresses: what two runs must agree on
std::vector<long long> shape(const Sets& S) {
    std::vector<long long> v = {S.rows.rows_cap, S.rows.fw_cap, S.adj.pending_cap, S.adj.chunk_cap,
                                S.adj.solve_ws_bytes, S.adj.cus, (long long)S.spans.chunks.size(), S.spans.slots,
                                (long long)S.pools.ev[0].size(), (long long)S.pools.ev[1].size(), S.pipe.n_streams,
                                S.pipe.n_events, g_live_dev, g_live_pinned, g_live_events, g_live_streams};
    for (auto& c : S.spans.chunks) v.push_back(c.cap), v.push_back(c.used);
    return v;
}

constexpr unsigned kReadbackFlags = hipEventDisableTiming | hipEventBlockingSync;
constexpr int kMaxDepth = 128;               // engine.h
constexpr size_t kPositionBytes = 40;        // sizeof(oamd_position)
// workspace bytes of the two solvers for n positions (the shape of solver.h's)
int64_t plain_bytes(int64_t n) { return 256 + n * 65 * 8; }
int64_t split_bytes(int64_t n) { return 256 + n * 1500; }

struct Step {
    const char* name;
    std::function<int(Sets&)> call;
};

const std::vector<Step>& steps() {
    static const std::vector<Step> v = {
        {"rows 3 x 10", [](Sets& S) { return S.rows.ensure(3, 10, kMaxDepth); }},
        {"rows grow to 17 x 10", [](Sets& S) { return S.rows.ensure(17, 10, kMaxDepth); }},
        {"rows fit", [](Sets& S) { return S.rows.ensure(5, 8, kMaxDepth); }},
        {"rows grow to 17 x 32 words", [](Sets& S) { return S.rows.ensure(17, 32, kMaxDepth); }},
        {"cut slots", [](Sets& S) { return S.cuts.ensure(64, 64, kReadbackFlags, "cut slots"); }},
        {"free-running slots", [](Sets& S) { return S.remaining.ensure(8, 32, kReadbackFlags, "free-running slots"); }},
        {"free-running slots again", [](Sets& S) { return S.remaining.ensure(8, 32, kReadbackFlags, "free-running slots"); }},
        {"adjudication, 100 positions, plain solver",
         [](Sets& S) { return S.adj.ensure(0, 100, kPositionBytes, plain_bytes(S.adj.chunk_for(100))); }},
        {"adjudication, 5000 positions, split solver",
         [](Sets& S) { return S.adj.ensure(0, 5000, kPositionBytes, split_bytes(S.adj.chunk_for(5000))); }},
        {"adjudication fits", [](Sets& S) { return S.adj.ensure(0, 64, kPositionBytes, plain_bytes(S.adj.chunk_for(64))); }},
        {"spans, first chunk", [](Sets& S) { return S.spans.reserve(SpanWindow::kChunk - 10, &S.span); }},
        {"spans across the chunk boundary", [](Sets& S) { return S.spans.reserve(20, &S.span); }},
        {"spans, a search larger than a chunk", [](Sets& S) { return S.spans.reserve(SpanWindow::kChunk + 7, &S.span); }},
        {"span window restart", [](Sets& S) { return S.spans.reset(); }},
        {"spans after the restart", [](Sets& S) { return S.spans.reserve(5, &S.span); }},
        {"timing pool 0", [](Sets& S) { return S.pools.ensure(0, 8); }},
        {"timing pool 1", [](Sets& S) { return S.pools.ensure(1, 8); }},
        {"timing pool 0 grows", [](Sets& S) { return S.pools.ensure(0, 20); }},
        {"streams, K = 2", [](Sets& S) { return S.pipe.ensure(2, 2); }},
        {"streams, K = 4", [](Sets& S) { return S.pipe.ensure(4, 4); }},
    };
    return v;
}

// one run of the scenario with the fail_at-th creating call failing; returns
// its final shape and, through *creates, the creating calls of a clean run
std::vector<long long> run(int fail_at, int* creates, std::vector<std::string>* k2_log, std::vector<std::string>* k4_log) {
    g_creates = g_failed = 0;
    g_fail_at = fail_at;
    std::vector<long long> end;
    const std::string tag = "fail_at " + std::to_string(fail_at) + ", ";
    {
        Sets S;
        for (const Step& st : steps()) {
            const std::vector<long long> before = state(S);
            const int failed_before = g_failed;
            g_log.clear();
            int rc = st.call(S);
            if (g_failed != failed_before) {
                check(rc == kStatusRuntime && !g_err.empty(), tag + st.name + ": a failed stub is reported");
                check(state(S) == before, tag + st.name + ": a failed call leaves every set as it was");
                g_log.clear();
                rc = st.call(S);  // the retry starts clean
            }
            check(rc == kStatusOk, tag + st.name + ": succeeds");
            if (!std::strcmp(st.name, "streams, K = 2") && k2_log) *k2_log = g_log;
            if (!std::strcmp(st.name, "streams, K = 4") && k4_log) *k4_log = g_log;
        }
        // what the sets hold is usable: the sanitizer checks the bounds
        std::memset(S.rows.policy.get(), 0, (size_t)(17 * 65 + RowBuffers::kEvalGuard) * sizeof(float));
        std::memset(S.rows.feat.get(), 0, (size_t)17 * 32 * sizeof(uint64_t));
        std::memset(S.rows.path.get(), 0, (size_t)17 * kMaxDepth * sizeof(int32_t));
        std::memset(S.adj.pending.get(), 0, 5000 * kPositionBytes);
        std::memset(S.adj.move_scores.get(), 0, (size_t)AdjudicateWorkspace::kChunk * 65 * sizeof(int32_t));
        std::memset(S.adj.solve_ws.get(), 0, (size_t)split_bytes(AdjudicateWorkspace::kChunk));
        std::memset(S.span, 0, 5 * 2 * sizeof(unsigned long long));
        std::memset(S.cuts.host.get(), 0, 64 * sizeof(int32_t));
        std::vector<std::pair<long long, long long>> iv;
        check(S.spans.intervals(&iv) == kStatusOk && iv.empty(), tag + "an untouched window holds no interval");
        end = shape(S);
        if (creates) *creates = g_creates;
    }
    check(g_live_dev == 0 && g_live_pinned == 0 && g_live_events == 0 && g_live_streams == 0,
          tag + "nothing is live after destruction");
    return end;
}

}  // namespace

int main() {
    int creates = 0;
    std::vector<std::string> k2, k4;
    const std::vector<long long> clean = run(0, &creates, &k2, &k4);
    check(g_failed == 0, "the clean run fails no stub");

    // the creation order and flags the schedules were measured with: the fork
    // event, the NN tokens, the idle stream BEFORE the group streams, a stream
    // and its join event per group, then the select events without the
    // system-scope fence
    const std::string ev = "event:" + std::to_string(hipEventDisableTiming);
    const std::string st = "stream:" + std::to_string(hipStreamNonBlocking);
    const std::string sel = "event:" + std::to_string(hipEventDisableTiming | hipEventDisableSystemFence);
    check(k2 == std::vector<std::string>{ev, ev, ev, ev, ev, st, st, ev, st, ev, sel, sel}, "creation order, K = 2");
    check(k4 == std::vector<std::string>{st, ev, st, ev, sel, sel}, "creation order, K = 2 -> 4");

    // every creating call of the scenario fails once; one past the last: none does
    int failed_runs = 0;
    for (int k = 1; k <= creates + 1; ++k) {
        int n = 0;
        const std::vector<long long> end = run(k, &n, nullptr, nullptr);
        check(end == clean, "fail_at " + std::to_string(k) + ": the run ends in the clean run's state");
        check(g_failed == (k <= creates ? 1 : 0), "fail_at " + std::to_string(k) + ": failing stubs");
        failed_runs += g_failed;
    }
    check(failed_runs == creates, "every creating call failed once");
    std::printf("%d creating calls, %d runs with one of them failing, %d checks, %d failures\n", creates, failed_runs,
                g_checks, g_failures);
    return g_failures ? 1 : 0;
}
