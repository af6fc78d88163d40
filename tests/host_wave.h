// host_wave.h -- a workgroup whose lanes are OS threads, for the host builds of the entropy cores (tests/inflate_host_main.cpp,
// bunzip2_host_main.cpp, bzip2_host_main.cpp; the mutation record is profiles/host_wave_mutations.md).  The including file defines
//   HW_T     threads of the workgroup          HW_WAVE  lanes per wave (a power of two, at most 64, dividing HW_T)
// and maps the core's macros to the calls below, each with HW_AT (the site's __FILE__, __LINE__).  hw::run(body) starts the HW_T threads
// on body(tid) and watches them; hw::tid is the calling thread's index.
//
// What the calls mean is taken from the kernels' own definitions (inflate_kernels.hip, bunzip2_kernels.hip, bzip2_kernels.hip):
//   sync       __syncthreads(): a pthread barrier over all HW_T threads
//   ballot     __ballot(p): bit l is set where lane l of the calling wave passed a true p
//   shfl_xor   __shfl_xor(v, m): v of lane ^ m (the caller's own where that lane is past the wave)
//   shfl_up    __shfl_up(v, d): v of lane - d, the caller's own in the lanes below d
//   readlane   __builtin_amdgcn_readlane(v, l): v of lane l; l must be equal in every lane
//   uni        __builtin_amdgcn_readfirstlane(x): the lowest lane's x -- and the run fails if any lane passed another value, which is what
//              "known to be equal in every lane" claims
//   lds_add / lds_or / lds_xor / lds_fetch_add   atomicAdd and its kin on a 32-bit word: relaxed __atomic builtins
// The four collectives go through one exchange array and one barrier per wave: every lane stores its value, the wave meets, every lane
// reads what it needs, the wave meets again.  Plain loads and stores of the core stay plain, so a thread sanitizer sees every pair of
// them that no barrier or collective separates.  (A collective orders the wave's memory traffic here, as lockstep execution does on the
// device; a barrier that only repeats that order cannot be told from none.)
//
// Every barrier and collective records its site.  All lanes that meet at one must have come from the same site: a lane that arrives from
// another line ends the run (exit 7).  A lane that waits for lanes that never come is found by the watchdog, which ends the run (exit 6)
// and prints every lane's last site.  No site of the three cores calls a collective from divergent code, so none is emulated with an
// explicit set of participating lanes.
#ifndef RPCC_HOST_WAVE_H
#define RPCC_HOST_WAVE_H

#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <time.h>
#include <unistd.h>

#ifndef HW_WATCHDOG_MS
#define HW_WATCHDOG_MS 20000    // no lane has left any barrier for this long: stuck
#endif
#define HW_AT __FILE__, __LINE__
#define HW_EXIT_UNIFORM 5
#define HW_EXIT_STUCK 6
#define HW_EXIT_SITE 7

namespace hw {

constexpr int T = HW_T, WAVE = HW_WAVE, NW = HW_T / HW_WAVE;
static_assert(WAVE >= 1 && WAVE <= 64 && (WAVE & (WAVE - 1)) == 0 && T % WAVE == 0, "waves of a power of two up to 64 lanes");

enum { RUNNING = 0, WAITING = 1, RETURNED = 2 };
struct Lane {                   // written by the lane, read by the watchdog: relaxed atomics
    const char *file;
    int line, state;
};
struct Site {
    const char *file;
    int line;
};
static Lane lanes[T];
static uint64_t progress;       // barriers left, over all lanes
static pthread_barrier_t group_barrier, wave_barrier[NW];
static uint64_t exchange[NW][WAVE];
static Site wave_site[NW][WAVE], group_site[2][T];     // group_site: by the parity of the barrier's number
static thread_local int tid = 0;
static thread_local unsigned group_count = 0;

static inline void dump(const char *what, const char *file, int line) {
    fprintf(stderr, "host_wave: %s at %s:%d (thread %d)\n", what, file, line, tid);
    for (int t = 0; t < T; ++t) {
        const char *f = __atomic_load_n(&lanes[t].file, __ATOMIC_RELAXED);
        const int st = __atomic_load_n(&lanes[t].state, __ATOMIC_RELAXED);
        fprintf(stderr, "  thread %4d (wave %2d lane %2d) %s %s:%d\n", t, t / WAVE, t % WAVE, st == WAITING ? "waits at" : st == RETURNED ? "returned, last" : "runs past",
                f ? f : "-", __atomic_load_n(&lanes[t].line, __ATOMIC_RELAXED));
    }
    fflush(stderr);
}
[[noreturn]] static inline void fail(int code, const char *what, const char *file, int line) {
    dump(what, file, line);
    _exit(code);
}

static inline void wait_at(pthread_barrier_t *b, const char *file, int line) {
    __atomic_store_n(&lanes[tid].file, file, __ATOMIC_RELAXED);
    __atomic_store_n(&lanes[tid].line, line, __ATOMIC_RELAXED);
    __atomic_store_n(&lanes[tid].state, (int)WAITING, __ATOMIC_RELAXED);
    pthread_barrier_wait(b);
    __atomic_store_n(&lanes[tid].state, (int)RUNNING, __ATOMIC_RELAXED);
    __atomic_fetch_add(&progress, 1, __ATOMIC_RELAXED);
}

static inline void sync(const char *file, int line) {
    Site *mine = group_site[group_count & 1u];
    mine[tid].file = file, mine[tid].line = line;
    wait_at(&group_barrier, file, line);
    if (mine[0].line != line || strcmp(mine[0].file, file)) fail(HW_EXIT_SITE, "threads met at one barrier from different sites", file, line);
    ++group_count;              // thread 0 writes this parity's slot again only after every thread has come to the next barrier
}

// every lane's v, in exchange[wave]; the wave's lanes came from one site
static inline const uint64_t *gather(uint64_t v, const char *file, int line) {
    const int w = tid / WAVE, l = tid % WAVE;
    exchange[w][l] = v;
    wave_site[w][l].file = file, wave_site[w][l].line = line;
    wait_at(&wave_barrier[w], file, line);
    if (wave_site[w][0].line != line || strcmp(wave_site[w][0].file, file)) fail(HW_EXIT_SITE, "lanes met at one collective from different sites", file, line);
    return exchange[w];
}
static inline void release(const char *file, int line) { wait_at(&wave_barrier[tid / WAVE], file, line); }

static inline unsigned long long ballot(bool p, const char *file, int line) {
    const uint64_t *x = gather(p ? 1u : 0u, file, line);
    unsigned long long m = 0;
    for (int l = 0; l < WAVE; ++l) m |= (unsigned long long)(x[l] & 1u) << l;
    release(file, line);
    return m;
}
template <class V>
static inline V shfl_xor(V v, int mask, const char *file, int line) {
    static_assert(sizeof(V) <= 8, "one exchange word");
    const uint64_t *x = gather((uint64_t)v, file, line);
    const int from = (tid % WAVE) ^ mask;
    const V r = from < WAVE ? (V)x[from] : v;
    release(file, line);
    return r;
}
template <class V>
static inline V shfl_up(V v, int delta, const char *file, int line) {
    static_assert(sizeof(V) <= 8, "one exchange word");
    const uint64_t *x = gather((uint64_t)v, file, line);
    const int l = tid % WAVE;
    const V r = l >= delta ? (V)x[l - delta] : v;
    release(file, line);
    return r;
}
static inline int readlane(int v, int from, const char *file, int line) {
    const uint64_t *x = gather((uint64_t)(uint32_t)v | (uint64_t)(uint32_t)from << 32, file, line);
    if ((int)(x[0] >> 32) != from) fail(HW_EXIT_UNIFORM, "the lane to read differs between the lanes", file, line);
    if (from < 0 || from >= WAVE) fail(HW_EXIT_UNIFORM, "the lane to read is not one of the wave", file, line);
    const int r = (int)(uint32_t)x[from];
    release(file, line);
    return r;
}
static inline int uni(int v, const char *file, int line) {
    const uint64_t *x = gather((uint64_t)(uint32_t)v, file, line);
    const int r = (int)(uint32_t)x[0];
    if (r != v) fail(HW_EXIT_UNIFORM, "a value said to be equal in every lane is not", file, line);
    release(file, line);
    return r;
}

static inline void lds_add(uint32_t *p, uint32_t v) { (void)__atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
static inline void lds_or(uint32_t *p, uint32_t v) { (void)__atomic_fetch_or(p, v, __ATOMIC_RELAXED); }
static inline void lds_xor(uint32_t *p, uint32_t v) { (void)__atomic_fetch_xor(p, v, __ATOMIC_RELAXED); }
static inline uint32_t lds_fetch_add(uint32_t *p, uint32_t v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }

struct Start {
    void (*body)(int);
    int tid;
};
static inline void *thread_main(void *arg) {
    const Start *s = (const Start *)arg;
    tid = s->tid;
    s->body(s->tid);
    __atomic_store_n(&lanes[tid].state, (int)RETURNED, __ATOMIC_RELEASE);
    return nullptr;
}

// body(tid) on HW_T threads; returns when all have returned.  The calling thread is the watchdog.
static inline void run(void (*body)(int)) {
    static Start starts[T];
    static pthread_t threads[T];
    pthread_barrier_init(&group_barrier, nullptr, T);
    for (int w = 0; w < NW; ++w) pthread_barrier_init(&wave_barrier[w], nullptr, WAVE);
    pthread_attr_t attr;
    pthread_attr_init(&attr);
    pthread_attr_setstacksize(&attr, 1 << 20);
    for (int t = 0; t < T; ++t) {
        starts[t].body = body, starts[t].tid = t;
        if (pthread_create(&threads[t], &attr, thread_main, &starts[t])) {
            fprintf(stderr, "host_wave: thread %d did not start\n", t);
            _exit(2);
        }
    }
    uint64_t seen = 0;
    int idle_ms = 0;
    for (;;) {
        int returned = 0, waiting = 0;
        for (int t = 0; t < T; ++t) {
            const int st = __atomic_load_n(&lanes[t].state, __ATOMIC_ACQUIRE);
            returned += st == RETURNED, waiting += st == WAITING;
        }
        if (returned == T) break;
        const struct timespec nap = {0, 20 * 1000 * 1000};
        nanosleep(&nap, nullptr);
        const uint64_t now = __atomic_load_n(&progress, __ATOMIC_RELAXED);
        idle_ms = now == seen ? idle_ms + 20 : 0;
        seen = now;
        // where every lane waits or has returned, none can come to free the others; otherwise a lane may be at work between two barriers
        if (idle_ms >= (returned + waiting == T ? 2000 : HW_WATCHDOG_MS)) fail(HW_EXIT_STUCK, "watchdog: no lane has left a barrier, some wait", "-", 0);
    }
    for (int t = 0; t < T; ++t) pthread_join(threads[t], nullptr);
}

}  // namespace hw

#endif  // RPCC_HOST_WAVE_H
