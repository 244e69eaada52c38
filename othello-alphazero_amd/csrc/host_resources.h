// Owners of the host layer's device resources (capi*.hip): device and pinned
// memory, events, streams, and the engine's resource sets built on them. An
// owner releases in its destructor; a set grows into locals and publishes
// them only when every creating call succeeded, so a failed call leaves the
// set as it was and a retry starts clean. Only the HIP runtime API and the
// standard library here (and schedule.h, host-only as well), so the host
// compiler alone builds it: tools/host_resources_check.cpp runs every set
// against counting stubs under the sanitizers (tests/test_cpu_endgame_split.py).
#pragma once

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "schedule.h"

namespace oamd {

// sets the calling thread's oamd_last_error message and returns code (capi.hip)
int fail(int code, const std::string& msg);
constexpr int kStatusOk = 0, kStatusRuntime = 3;  // OAMD_OK, OAMD_RUNTIME (capi_internal.h checks)

#define HIPCHK(expr)                                                                         \
    do {                                                                                     \
        hipError_t _e = (expr);                                                              \
        if (_e != hipSuccess)                                                                \
            return ::oamd::fail(::oamd::kStatusRuntime, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

// ---------------------------------------------------------------------------
// owners: move-only, get(), one creating call, released by the destructor
// ---------------------------------------------------------------------------
template <typename H, hipError_t (*Release)(H)>
class Owner {
  public:
    Owner() = default;
    Owner(Owner&& o) noexcept : h_(o.h_) { o.h_ = H{}; }
    Owner& operator=(Owner&& o) noexcept {
        if (this != &o) {
            reset();
            h_ = o.h_;
            o.h_ = H{};
        }
        return *this;
    }
    ~Owner() { reset(); }
    void reset() {
        if (h_) (void)Release(h_);
        h_ = H{};
    }

  protected:
    H h_{};
};

// n elements of device memory (n = 0: none, get() stays null)
template <typename T>
struct DeviceBuf : Owner<void*, hipFree> {
    T* get() const { return static_cast<T*>(h_); }
    int alloc(size_t n) {
        reset();
        if (n == 0) return kStatusOk;
        const hipError_t e = hipMalloc(&h_, n * sizeof(T));
        if (e == hipSuccess) return kStatusOk;
        h_ = nullptr;
        return fail(kStatusRuntime, std::string("hipMalloc: ") + hipGetErrorString(e));
    }
};

// n elements of pinned host memory
template <typename T>
struct PinnedBuf : Owner<void*, hipHostFree> {
    T* get() const { return static_cast<T*>(h_); }
    int alloc(size_t n, const char* what) {
        reset();
        if (hipHostMalloc(&h_, n * sizeof(T), hipHostMallocDefault) == hipSuccess) return kStatusOk;
        h_ = nullptr;
        return fail(kStatusRuntime, std::string(what) + ": hipHostMalloc failed");
    }
};

struct Event : Owner<hipEvent_t, hipEventDestroy> {
    hipEvent_t get() const { return h_; }
    int create(unsigned flags, const char* what) {
        reset();
        if (hipEventCreateWithFlags(&h_, flags) == hipSuccess) return kStatusOk;
        h_ = nullptr;
        return fail(kStatusRuntime, std::string(what) + ": hipEventCreate failed");
    }
};

struct Stream : Owner<hipStream_t, hipStreamDestroy> {
    hipStream_t get() const { return h_; }
    int create(unsigned flags, const char* what) {
        reset();
        if (hipStreamCreateWithFlags(&h_, flags) == hipSuccess) return kStatusOk;
        h_ = nullptr;
        return fail(kStatusRuntime, std::string(what) + ": hipStreamCreate failed");
    }
};

// compute units of a device, at least 1 (the solver's grid)
inline int device_cus(int device, int* cus) {
    *cus = 0;
    HIPCHK(hipDeviceGetAttribute(cus, hipDeviceAttributeMultiprocessorCount, device));
    if (*cus < 1) *cus = 1;
    return kStatusOk;
}

// ---------------------------------------------------------------------------
// the engine's resource sets
// ---------------------------------------------------------------------------

// Per-row buffers of the search (EngineView), sized for rows_cap rows of
// fw_cap feature words; they only grow.
struct RowBuffers {
    static constexpr int kEvalGuard = 16;  // guard floats behind policy / value
    static constexpr int kEvalGuardByte = 0x5A;
    int64_t rows_cap = 0;
    int fw_cap = 0;
    DeviceBuf<int32_t> leaf, depth, trans, path;
    DeviceBuf<uint64_t> feat;
    DeviceBuf<float> policy, value;
    DeviceBuf<uint8_t> flags;
    // evaluation lists of the native search (tree_search.h append_rows): the rows of
    // non-terminal leaves per pipeline group
    DeviceBuf<int32_t> rowlist;
    DeviceBuf<int32_t> tstate;  // per game and virtual thread: batches selected, pending (k_tree)
    DeviceBuf<int32_t> exact;   // per row: the exact-leaf flag of the selected leaf (engine.h)

    // max_depth: path slots per row (engine.h kMaxDepth). A shape that does not
    // fit is allocated whole beside the old set, which is released on success.
    bool fits(int64_t rows, int fw) const { return rows <= rows_cap && fw <= fw_cap; }
    int ensure(int64_t rows, int fw, int max_depth) {
        if (fits(rows, fw)) return kStatusOk;
        RowBuffers t;
        int rc;
        if ((rc = t.leaf.alloc(rows)) || (rc = t.depth.alloc(rows)) || (rc = t.trans.alloc(rows)) ||
            (rc = t.path.alloc(rows * max_depth)) || (rc = t.feat.alloc(rows * fw)) ||
            (rc = t.policy.alloc(rows * 65 + kEvalGuard)) || (rc = t.value.alloc(rows + kEvalGuard)) ||
            (rc = t.flags.alloc(rows)) || (rc = t.rowlist.alloc(rows)) || (rc = t.tstate.alloc(rows)) ||
            (rc = t.exact.alloc(rows)))
            return rc;
        HIPCHK(hipMemset(t.exact.get(), 0, rows * sizeof(int32_t)));  // no row pending
        HIPCHK(hipMemset(t.policy.get(), 0, rows * 65 * sizeof(float)));
        HIPCHK(hipMemset(t.value.get(), 0, rows * sizeof(float)));
        // guard words behind both (oamd_debug_eval_guards): no launch writes them
        HIPCHK(hipMemset(t.policy.get() + rows * 65, kEvalGuardByte, kEvalGuard * sizeof(float)));
        HIPCHK(hipMemset(t.value.get() + rows, kEvalGuardByte, kEvalGuard * sizeof(float)));
        t.rows_cap = rows;
        t.fw_cap = fw;
        *this = std::move(t);
        return kStatusOk;
    }
};

// Values the host reads back late: a device array, its pinned host mirror,
// and an event per (slot, pipeline group) behind each copy into the mirror.
struct ReadbackSlots {
    static constexpr int kSlots = 4;
    DeviceBuf<int32_t> dev;
    PinnedBuf<int32_t> host;
    Event ev[kSlots][kMaxPipeline];

    ReadbackSlots() = default;
    ReadbackSlots(ReadbackSlots&&) = default;
    ReadbackSlots& operator=(ReadbackSlots&&) = default;
    ~ReadbackSlots() {
        if (dev.get()) (void)hipDeviceSynchronize();  // no copy into the pinned mirror in flight
    }
    int ensure(size_t dev_words, size_t host_words, unsigned event_flags, const char* what) {
        if (dev.get()) return kStatusOk;
        ReadbackSlots t;
        int rc;
        if ((rc = t.dev.alloc(dev_words)) || (rc = t.host.alloc(host_words, what))) return rc;
        for (auto& row : t.ev)
            for (auto& x : row)
                if ((rc = x.create(event_flags, what))) return rc;
        *this = std::move(t);
        return kStatusOk;
    }
};

// Adjudication: the pending positions of one call (one slot
// per `finished` word, all-zero where no game ended) and what the solver needs
// for one chunk of them. Engine-owned, grown lazily; hipFree waits for the
// device, so growing never pulls a buffer from under queued work.
struct AdjudicateWorkspace {
    static constexpr int64_t kChunk = 4096;  // positions per solver launch
    DeviceBuf<unsigned char> pending;        // pending_cap positions (oamd_position)
    int64_t pending_cap = 0;
    DeviceBuf<int32_t> move_scores;  // chunk x 65
    DeviceBuf<int32_t> score;        // chunk
    DeviceBuf<int32_t> flags;        // chunk
    DeviceBuf<char> solve_ws;
    int64_t chunk_cap = 0, solve_ws_bytes = 0;
    int cus = 0;
    Event ev[2];  // around the last resolve step, once oamd_engine_adjudicate_ms was called
    bool want_ms = false, timed = false;
    int64_t resolves = 0;

    // positions per solver launch once n pending positions fit
    int64_t chunk_for(int64_t n) const { return std::max(chunk_cap, std::min(n, kChunk)); }
    // n pending positions of position_bytes each, and solve_bytes of solver
    // workspace (solver.h, for chunk_for(n) positions)
    int ensure(int device, int64_t n, size_t position_bytes, int64_t solve_bytes) {
        Event e0, e1;
        int c = cus, rc;
        if (!ev[0].get())
            if ((rc = e0.create(hipEventDefault, "adjudication")) || (rc = e1.create(hipEventDefault, "adjudication")) ||
                (rc = device_cus(device, &c)))
                return rc;
        DeviceBuf<unsigned char> p;
        DeviceBuf<int32_t> m, s, f;
        DeviceBuf<char> w;
        const int64_t chunk = chunk_for(n);
        if (n > pending_cap && (rc = p.alloc((size_t)n * position_bytes))) return rc;
        if (chunk > chunk_cap &&
            ((rc = m.alloc((size_t)chunk * 65)) || (rc = s.alloc((size_t)chunk)) || (rc = f.alloc((size_t)chunk))))
            return rc;
        if (solve_bytes > solve_ws_bytes && (rc = w.alloc((size_t)solve_bytes))) return rc;
        if (e0.get()) {
            ev[0] = std::move(e0);
            ev[1] = std::move(e1);
            cus = c;
        }
        if (p.get()) {
            pending = std::move(p);
            pending_cap = n;
        }
        if (m.get()) {
            move_scores = std::move(m);
            score = std::move(s);
            flags = std::move(f);
            chunk_cap = chunk;
        }
        if (w.get()) {
            solve_ws = std::move(w);
            solve_ws_bytes = solve_bytes;
        }
        return kStatusOk;
    }
};

// NN busy time (oamd_engine_nn_busy): while timing is enabled, EVERY
// ResNet launch of a native search records its execution interval
// (kernel-side span, launch_resnet_packed: ~start, end in 100 MHz ticks)
// in a window of slots, zeroed when allocated and when the window
// restarts; the busy time is the union over the whole window (launches of
// the pipeline groups' searches overlap in time, and the groups drift
// apart over whole games, so per-search unions would count shared time
// twice). A search's slots are contiguous: [group][round][launch], in one
// chunk of at least kChunk slots (larger when one search needs more).
// Chunks that no search reserves in any more are copied to the host once
// (ticks); a window of more than kWindow slots stops recording
// and makes oamd_engine_nn_busy fail (its launches would be missing).
struct SpanWindow {
    static constexpr int64_t kChunk = 1 << 15;   // slots (2 x u64) per chunk
    static constexpr int64_t kWindow = 1 << 23;  // most slots of one window (128 MiB)
    struct Chunk {
        DeviceBuf<unsigned long long> p;
        int64_t cap = 0, used = 0;
    };
    std::vector<Chunk> chunks;
    int64_t slots = 0;    // slots reserved in this window
    int64_t dropped = 0;  // launches of this window that found no slot
    size_t copied = 0;    // leading chunks already folded into ticks
    std::vector<std::pair<long long, long long>> ticks;  // their intervals (ticks)

    // n contiguous span slots for one search
    int reserve(int64_t n, unsigned long long** out) {
        *out = nullptr;
        if (n <= 0) return kStatusOk;
        if (slots + n > kWindow) {  // not recorded: nn_busy reports it
            dropped += n;
            return kStatusOk;
        }
        if (chunks.empty() || chunks.back().used + n > chunks.back().cap) {
            Chunk c;
            c.cap = std::max(kChunk, n);
            if (int rc = c.p.alloc((size_t)2 * c.cap)) return rc;
            if (hipMemset(c.p.get(), 0, sizeof(unsigned long long) * 2 * c.cap) != hipSuccess)
                return fail(kStatusRuntime, "span window: hipMemset failed");
            chunks.push_back(std::move(c));
        }
        Chunk& c = chunks.back();
        *out = c.p.get() + 2 * c.used;
        c.used += n;
        slots += n;
        return kStatusOk;
    }
    // restart the window: every launch that may still write a slot is done
    int reset() {
        if (chunks.empty() && !dropped) return kStatusOk;
        HIPCHK(hipDeviceSynchronize());
        chunks.clear();
        slots = dropped = 0;
        copied = 0;
        ticks.clear();
        return kStatusOk;
    }
    // the window's recorded intervals (ticks); waits for the device
    int intervals(std::vector<std::pair<long long, long long>>* iv) {
        HIPCHK(hipDeviceSynchronize());  // every launch of the window has written its slot
        auto read = [&](const Chunk& c, std::vector<std::pair<long long, long long>>* to) -> int {
            std::vector<unsigned long long> sp((size_t)2 * c.used);
            if (c.used)
                HIPCHK(hipMemcpy(sp.data(), c.p.get(), sizeof(unsigned long long) * 2 * c.used, hipMemcpyDeviceToHost));
            for (int64_t i = 0; i < c.used; ++i)  // start stored complemented (an atomicMin on zeroed slots)
                if (sp[2 * i + 1]) to->emplace_back((long long)~sp[2 * i], (long long)sp[2 * i + 1]);
            return kStatusOk;
        };
        // chunks before the last one are complete: fold them in once
        for (; copied + 1 < chunks.size(); ++copied) {
            if (int rc = read(chunks[copied], &ticks)) return rc;
            chunks[copied].p.reset();
        }
        *iv = ticks;
        if (!chunks.empty())
            if (int rc = read(chunks.back(), iv)) return rc;
        return kStatusOk;
    }
};

// Timing events of the native searches, in two pools used in turn, so a
// search never waits for the previous one's events (default flags: they time)
struct TimingPools {
    std::vector<Event> ev[2];
    // at least n events in pool p
    int ensure(int p, size_t n) {
        std::vector<Event> more;
        while (ev[p].size() + more.size() < n) {
            more.emplace_back();
            if (int rc = more.back().create(hipEventDefault, "timing")) return rc;
        }
        for (auto& x : more) ev[p].push_back(std::move(x));
        return kStatusOk;
    }
};

// K streams (one per pipeline group, or per virtual thread of the single-game
// thread split) with their fork / join events, the NN tokens, and a select
// event per virtual thread of the thread split. The creation order is part of
// the schedule's measured behaviour (idle): keep it.
struct PipelineStreams {
    static constexpr int kMaxChains = 4;
    int n_streams = 0;
    int n_events = 0;  // sel_ev created
    Event fork_ev;
    // NN tokens: the pipeline groups' ResNet launches form nn_chains chains
    // (group k in chain k % nn_chains); launches of one chain run one after
    // another (a token event passed between the group streams), each owning
    // every CU while the other groups' tree kernels run beside it; chains run
    // concurrently (1 = every launch serialised). The default is one chain
    // per group (2 groups, 2 chains): a group's launch starts as soon as its
    // selection is done
    Event nn_token[kMaxChains];
    // never used, but created ahead of the group / thread streams: without it the single-game thread split's
    // 800-simulation search measured 10.0 instead of 5.1 ms (profiles/schedule_refactor/ab.json)
    Stream idle;
    Stream stream[kMaxPipeline];
    Event join_ev[kMaxPipeline];
    Event sel_ev[kMaxPipeline];

    // at least K streams and nev select events
    int ensure(int K, int nev) {
        if (K <= 1 && nev <= 1) return kStatusOk;
        const char* what = "pipeline streams";
        Event f, tok[kMaxChains], je[kMaxPipeline], se[kMaxPipeline];
        Stream id, st[kMaxPipeline];
        int rc;
        if (!fork_ev.get() && (rc = f.create(hipEventDisableTiming, what))) return rc;
        for (int c = 0; c < kMaxChains; ++c)
            if (!nn_token[c].get() && (rc = tok[c].create(hipEventDisableTiming, what))) return rc;
        if (!idle.get() && (rc = id.create(hipStreamNonBlocking, what))) return rc;
        for (int k = n_streams; k < K; ++k)
            if ((rc = st[k].create(hipStreamNonBlocking, what)) || (rc = je[k].create(hipEventDisableTiming, what)))
                return rc;
        // sel_ev only orders kernels of this device (the split schedule's tree
        // operations): no system-scope fence (its host-visibility cache
        // maintenance) on the cross-stream path of every round
        for (int k = n_events; k < nev; ++k)
            if ((rc = se[k].create(hipEventDisableTiming | hipEventDisableSystemFence, what))) return rc;
        if (f.get()) fork_ev = std::move(f);
        for (int c = 0; c < kMaxChains; ++c)
            if (tok[c].get()) nn_token[c] = std::move(tok[c]);
        if (id.get()) idle = std::move(id);
        for (int k = n_streams; k < K; ++k) {
            stream[k] = std::move(st[k]);
            join_ev[k] = std::move(je[k]);
        }
        for (int k = n_events; k < nev; ++k) sel_ev[k] = std::move(se[k]);
        n_streams = std::max(n_streams, K);
        n_events = std::max(n_events, nev);
        return kStatusOk;
    }
};

}  // namespace oamd
