// call.cpp — what every library call shares: the stream it runs on and the order between streams,
// the host profile and kernel-time marks, the completion word its last kernel raises and the host
// waits for, and the error word a kernel that gave up waiting for a peer leaves behind.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <unistd.h>

#include "coll_internal.h"
#include "log.h"

namespace mv2 {

int log_rank() { return world().grank; }  // the job's rank (a node's local rank 0 is not unique)
bool log_debug_on() {
    static int on = -1;
    if (on < 0) {
        const char *v = getenv("MV2AMD_DEBUG");
        on = (v && *v && *v != '0') ? 1 : 0;
    }
    return on == 1;
}

// The stream of a call.  Every collective kernel of this process shares the arenas, flag
// epochs and slot parities, which the host hands out in call order, so the kernels must also
// run in call order whatever stream each call names.  One event carries the order: a call on
// a caller's stream records it on that stream when it ends (stream_tail — the caller may
// destroy the stream afterwards, so the library never touches it again), a call on the
// library's own stream records it lazily when the next call names another stream; a call on
// a stream other than the previous one first waits for it.  Calls that stay on one stream
// pay nothing for the order.  (A caller's stream handle reused after hipStreamDestroy is
// safe: the destroy drains the stream's queue first.)
hipStream_t pick_stream(void *s) {
    World &w = world();
    hipStream_t st = s ? (hipStream_t)s : w.stream;
    if (st == w.stream) w.stream_hip_busy = true;  // runtime/aql.cpp consults HIP before its next dispatch
    if (w.graph) return st;  // graph lane: disjoint arenas and epochs, ordered by the graph itself
    if (w.last_st && st != w.last_st) {
        if (!w.sw_ev) hipEventCreateWithFlags(&w.sw_ev, hipEventDisableTiming);
        if (w.sw_ev) {
            if (w.last_st == w.stream && st != w.stream) hipEventRecord(w.sw_ev, w.stream);
            hipStreamWaitEvent(st, w.sw_ev, 0);
        }
    }
    w.last_st = st;
    return st;
}
void stream_tail(hipStream_t st) {
    World &w = world();
    if (st == w.stream || w.graph) return;
    if (!w.sw_ev) hipEventCreateWithFlags(&w.sw_ev, hipEventDisableTiming);
    if (w.sw_ev) hipEventRecord(w.sw_ev, st);
}

// Host-side profile of blocking calls (MV2AMD_HOST_PROFILE=1, printed at
// MPI_Finalize): time from API entry to the kernel launch (argument checks,
// plan, staging), inside hipLaunchKernel, and from the launch to the
// completion word (kernel run + peers' arrival).
struct HostProf {
    int on = -1;
    uint64_t calls = 0, pre_ns = 0, launch_ns = 0, wait_ns = 0;
    uint64_t t_entry = 0, t_l0 = 0, t_l1 = 0;
};
static HostProf g_hp;
uint64_t now_ns() {
    timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return (uint64_t)t.tv_sec * 1000000000ull + (uint64_t)t.tv_nsec;
}
static inline bool hp_on() {
    if (g_hp.on < 0) {
        const char *v = getenv("MV2AMD_HOST_PROFILE");
        g_hp.on = v && atoi(v) > 0 ? atoi(v) : 0;
    }
    return g_hp.on;
}
static bool g_call_start = true;  // tmark0: record ev0 at the first launch of this API call
void hp_entry() {
    g_call_start = true;
    beacon(BC_ENTRY, true);
    if (hp_on()) g_hp.t_entry = now_ns();
}
static inline void hp_done() {
    if (!hp_on() || !g_hp.t_entry || !g_hp.t_l1) return;
    const uint64_t t = now_ns();
    // MV2AMD_HOST_PROFILE=k > 1: the first k - 1 calls (warm-up, first-launch code loading) are
    // left out of the means
    static uint64_t seen = 0;
    if (++seen < (uint64_t)g_hp.on) {
        g_hp.t_entry = g_hp.t_l0 = g_hp.t_l1 = 0;
        return;
    }
    ++g_hp.calls;
    g_hp.pre_ns += g_hp.t_l0 - g_hp.t_entry;
    g_hp.launch_ns += g_hp.t_l1 - g_hp.t_l0;
    g_hp.wait_ns += t - g_hp.t_l1;
    g_hp.t_entry = g_hp.t_l0 = g_hp.t_l1 = 0;
}
void host_prof_report() {
    if (!hp_on() || !g_hp.calls) return;
    const double c = (double)g_hp.calls * 1e3;
    fprintf(stderr, "[mv2amd rank %d] host profile: %llu calls, entry->launch %.3f us, launch %.3f us, launch->done %.3f us\n",
            world().rank, (unsigned long long)g_hp.calls, g_hp.pre_ns / c, g_hp.launch_ns / c, g_hp.wait_ns / c);
}


// Completion word for the kernel about to be launched on `st` as the call's
// last stream operation (only the library's own stream; cleared again by
// any copy enqueued after it, see enq_copy).
// Test hooks (mv2h_set_tuning): "withhold_done" = k makes the next k armed kernels run without
// their word (the host still waits for it: the missed-word path of wait_done), "fake_split" = k
// marks the next k words as raised by a kernel whose block groups ran on several XCDs.
static int g_withhold_done = 0, g_fake_split = 0;
void withhold_done(int k) { g_withhold_done = k; }
void fake_split(int k) { g_fake_split = k; }

Done arm_done(hipStream_t st) {
    World &w = world();
    if (w.sync_mode != 0 || !w.done_flag || st != w.stream || w.enqueue) return Done{nullptr, nullptr, 0};
    w.pending = ++w.done_seq;
    if (g_fake_split > 0) {
        --g_fake_split;
        __atomic_store_n(w.done_flag + 1, w.pending, __ATOMIC_RELEASE);
    }
    if (g_withhold_done > 0) {
        --g_withhold_done;
        return Done{nullptr, nullptr, 0};
    }
    return Done{w.done_ctr, w.done_flag, w.pending};
}

hipError_t enq_copy(void *dst, const void *src, size_t bytes, hipStream_t st) {
    beacon(BC_COPY_OUT);
    world().pending = 0;
    return hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, st);
}

// A completion word whose kernel ran a block group over more than one XCD (device_util.h
// block_done wrote its seq into done_flag[1] too): that group's L2 write-back did not cover every
// block, so the call completes with a stream synchronisation (the kernel's end releases every
// XCD's L2) before the host returns.  Counted (done_xcd_split) and reported once per process.
hipError_t settle_split(hipStream_t st) {
    World &w = world();
    const uint64_t s = __atomic_load_n(w.done_flag + 1, __ATOMIC_ACQUIRE);
    if (s <= w.split_seen) return hipSuccess;
    w.split_seen = s;
    if (w.done_xcd_split++ == 0)
        fprintf(stderr, "[mv2amd rank %d] warning: a kernel's workgroups of one group ran on several XCDs; "
                        "completing such calls with a stream synchronisation (counted in done_xcd_split)\n",
                log_rank());
    return hipStreamSynchronize(st);
}

// Wait for the armed completion word; fall back to the stream when the
// kernel ended without raising it (should not happen: counters are reset).
// The word is the normal path: the stream is consulted only once the word is
// 200 us late, then every 100 us (a hipStreamQuery costs ~3 us of host time,
// and one in flight when the word lands delays the return by that much).
// Every fallback is counted and the first missed word of the process is reported (a missed word
// would otherwise be invisible in every record): done_queried -- the stream was consulted at least
// once (any call whose kernel runs longer than 200 us, e.g. a 256 MiB allreduce on a shared GPU);
// done_late -- the stream already reported the kernel finished when the word was seen (the word
// trailed the kernel's end); done_missed -- the kernel had ended without raising the word.
hipError_t wait_done(hipStream_t st, uint64_t want) {
    World &w = world();
    uint64_t next_query = 0;
    bool queried = false;
    for (unsigned spins = 0;; ++spins) {
        if (__atomic_load_n(w.done_flag, __ATOMIC_ACQUIRE) >= want) return settle_split(st);
        if ((spins & 255u) == 0) {
            const uint64_t t = now_ns();
            if (!next_query) next_query = t + 200000;
            if (t < next_query) continue;
            next_query = t + 100000;
            if (!queried) {
                queried = true;
                ++w.done_queried;
            }
            const hipError_t q = hipStreamQuery(st);
            if (q == hipErrorNotReady) continue;
            if (__atomic_load_n(w.done_flag, __ATOMIC_ACQUIRE) >= want) {
                if (q == hipSuccess) ++w.done_late;
                return settle_split(st);
            }
            if (q == hipSuccess) {
                if (w.done_missed++ == 0)
                    fprintf(stderr, "[mv2amd rank %d] warning: a kernel finished without raising its completion word "
                                    "(call %llu); completing by stream synchronisation, counters reset (counted in done_missed)\n",
                            log_rank(), (unsigned long long)want);
                hipMemsetAsync(w.done_ctr, 0, kDoneBytes, st);
                return hipStreamSynchronize(st);
            }
            return q;
        }
    }
}

void log_epochs(uint64_t lo, uint64_t hi, hipStream_t st) {
    World &w = world();
    w.epoch_log[w.epoch_pos++ % 8] = World::EpochRec{w.api_calls, lo, hi, st != w.stream};
}

// The waited slot of every rank in `mask` as it is in memory now (read by a copy on a stream of
// its own, after the kernel gave up): a value above the one the kernel last saw means its loads
// were served stale; the same value means the peer's flag store never landed.
static void report_slot_now(int blk, unsigned mask) {
    World &w = world();
    if (!w.sig || blk < 0 || blk >= kMaxBlocks) return;
    hipStream_t s = nullptr;
    if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) {
        (void)hipGetLastError();
        return;
    }
    uint64_t *h = nullptr;
    if (hipHostMalloc((void **)&h, kMaxRanks * sizeof(uint64_t), hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        hipStreamDestroy(s);
        return;
    }
    bool ok = true;
    for (int j = 0; j < kMaxRanks && ok; ++j)
        if ((mask >> j) & 1u)
            ok = hipMemcpyAsync(h + j, w.sig + (size_t)j * kMaxBlocks + blk, sizeof(uint64_t), hipMemcpyDeviceToHost, s) ==
                 hipSuccess;
    const uint64_t t0 = now_ns();
    hipError_t q = hipErrorNotReady;
    while (ok && (q = hipStreamQuery(s)) == hipErrorNotReady && now_ns() - t0 < 2000000000ull) usleep(100);
    if (ok && q == hipSuccess) {
        char line[256];
        int o = 0;
        for (int j = 0; j < kMaxRanks && o < (int)sizeof(line) - 40; ++j)
            if ((mask >> j) & 1u) o += snprintf(line + o, sizeof(line) - o, " r%d=%llu", j, (unsigned long long)h[j]);
        line[o] = 0;
        MV2_ERR("  the waited slot now (host copy):%s", line);
    }
    (void)hipGetLastError();
    if (q != hipErrorNotReady) {  // a copy still in flight keeps its buffers
        hipHostFree(h);
        hipStreamDestroy(s);
    }
}

// A kernel gave up waiting for a peer (device_util.h wait_mask): report what it waited for —
// the epoch, the ranks and the flag values it last saw from each, next to this rank's host
// counters — so a failure tells a late peer (flag = an earlier epoch of the same call
// sequence) from a peer whose call sequence diverged (flags of another call's epochs).
int check_err_word() {
    World &w = world();
    if (!w.h_err || !__atomic_load_n(w.h_err, __ATOMIC_ACQUIRE)) return 0;
    int *e = w.h_err;
    const uint64_t ep = (uint64_t)(uint32_t)e[2] | ((uint64_t)(uint32_t)e[3] << 32);
    char seen[256];
    int o = 0;
    for (int j = 0; j < kMaxRanks && o < (int)sizeof(seen) - 40; ++j)
        if (((unsigned)e[4] >> j) & 1u) {
            const uint64_t v = (uint64_t)(uint32_t)e[8 + 2 * j] | ((uint64_t)(uint32_t)e[9 + 2 * j] << 32);
            o += snprintf(seen + o, sizeof(seen) - o, " r%d=%llu", j, (unsigned long long)v);
        }
    seen[o] = 0;
    MV2_ERR("device collective timed out waiting for a peer (MV2AMD_TIMEOUT_S): workgroup %d waited for epoch "
            "%llu from ranks 0x%x; flags seen:%s; host epoch %llu, round %llu, one-shot calls %llu, call %llu",
            e[1], (unsigned long long)ep, (unsigned)e[4], seen, (unsigned long long)w.epoch, (unsigned long long)w.round,
            (unsigned long long)w.os_calls, (unsigned long long)w.done_seq);
    {
        char line[512];
        int o = 0;
        for (unsigned k = w.epoch_pos > 8 ? w.epoch_pos - 8 : 0; k < w.epoch_pos && o < (int)sizeof(line) - 80; ++k) {
            const World::EpochRec &r = w.epoch_log[k % 8];
            o += snprintf(line + o, sizeof(line) - o, " %llu:%llu-%llu%s%s", (unsigned long long)r.call,
                          (unsigned long long)r.lo, (unsigned long long)r.hi, r.user_stream ? "(caller's stream)" : "",
                          r.lo <= ep && ep <= r.hi ? "<-" : "");
        }
        line[o] = 0;
        MV2_ERR("  this rank's last launches with flag epochs (call:epochs, <- the waiting one):%s", line);
    }
    report_slot_now(e[1], (unsigned)e[4]);
    // where each late peer's host is now (its beacon in the control segment), next to this rank's
    if (w.shm) {
        const uint64_t t = now_ns();
        for (int j = 0; j < w.size && j < kMaxRanks; ++j) {
            const uint64_t v = (uint64_t)(uint32_t)e[8 + 2 * j] | ((uint64_t)(uint32_t)e[9 + 2 * j] << 32);
            if (j != w.rank && !((((unsigned)e[4] >> j) & 1u) && v < ep)) continue;
            const uint64_t b = w.shm->r[j].beacon.load(std::memory_order_relaxed);
            const uint64_t bt = w.shm->r[j].beacon_ns.load(std::memory_order_relaxed);
            MV2_ERR("  %s local rank %d: library call %llu, %s, for %.1f ms", j == w.rank ? "this is" : "late peer:", j,
                    (unsigned long long)(b >> 8), beacon_name((int)(b & 0xff)), bt && t > bt ? (t - bt) / 1e6 : 0.0);
            beacon_report(j, t);
        }
    }
    memset(e + 1, 0, (kErrWords - 1) * sizeof(int));
    __atomic_store_n(e, 0, __ATOMIC_RELEASE);
    return E_OTHER;
}

int finish(hipStream_t st, bool timed) {
    World &w = world();
    hipError_t e;
    const uint64_t want = w.pending;
    w.pending = 0;
    stream_tail(st);
    if (w.enqueue) return 0;  // stream-ordered: the caller's stream carries the completion
    if (w.defer && want) {  // nonblocking initiation: the ticket waits later
        w.deferred = want;
        return 0;
    }
    if (w.defer) w.deferred = 0;
    beacon(BC_WAIT);
    if (want) {
        e = wait_done(st, want);
        if (e == hipSuccess && timed) e = hipEventSynchronize(w.ev1);
    } else {
        e = hipStreamSynchronize(st);
    }
    if (e != hipSuccess) {
        MV2_ERR("hipStreamSynchronize failed: %s", hipGetErrorString(hipGetLastError()));
        return E_INTERN;
    }
    if (timed) {
        float ms = 0.f;
        hipEventElapsedTime(&ms, w.ev0, w.ev1);
        w.last_ms = ms;
    }
    if (check_err_word()) return E_OTHER;
    beacon(BC_DONE);
    hp_done();
    return 0;
}

// kernel-time events bracket the call's first launch to its last (calls made of several
// launches: ring main part + remainder, staged copies)
void tmark0(hipStream_t st) {
    if (g_call_start) beacon(BC_LAUNCH);
    if (world().timing && g_call_start) hipEventRecord(world().ev0, st);
    g_call_start = false;
    if (hp_on() && g_hp.t_entry && !g_hp.t_l0) g_hp.t_l0 = now_ns();
}
void tmark1(hipStream_t st) {
    beacon(BC_LAUNCHED);
    if (world().timing) hipEventRecord(world().ev1, st);
    if (hp_on() && g_hp.t_entry) g_hp.t_l1 = now_ns();
}

// 1 = device memory (hipMalloc / IPC-importable), 0 = anything else
int is_device(const void *p) {
    if (!p) return 0;
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        hipGetLastError();
        return 0;
    }
    return a.type == hipMemoryTypeDevice ? 1 : 0;
}

// The call's last copy, device to device, as a copy kernel that raises the completion word:
// a hipMemcpyAsync cannot raise it, and without it finish() falls back to a stream
// synchronisation (several us at small sizes).  Other copies keep enq_copy.
hipError_t enq_copy_last(void *dst, const void *src, size_t bytes, hipStream_t st) {
    constexpr size_t kKernelCopyMax = (size_t)4 << 20;
    if (bytes && bytes <= kKernelCopyMax && is_device(dst) && is_device(src)) {
        const Done d = arm_done(st);
        if (d.flag) {
            beacon(BC_COPY_OUT);
            if (launch_pack_strided(src, dst, 1, bytes, bytes, 0, st, d) == 0) return hipSuccess;
            world().pending = 0;  // no kernel will raise the word: finish() must not wait for it
            MV2_ERR("launching the result copy-out failed: %s", hipGetErrorString(hipGetLastError()));
            return hipErrorLaunchFailure;
        }
    }
    return enq_copy(dst, src, bytes, st);
}

int kind_supported(const DtypeInfo *dt) {
    if (!dt) return E_TYPE;
    if (dt->kind == K_LDOUBLE) {
        MV2_ERR("%s: x87 80-bit long double has no gfx950 representation (not supported on device)", dt->name);
        return E_TYPE;
    }
    return 0;
}

int check_op_dtype(int op, int dtype, const DtypeInfo **out) {
    const DtypeInfo *dt = dtype_lookup(dtype);
    if (!dt) return E_TYPE;
    if (!is_builtin_op(op)) return E_OP;
    if (!op_valid_for_groups(op_index(op), dt->groups)) return E_OP;
    *out = dt;
    return 0;
}

}  // namespace mv2
