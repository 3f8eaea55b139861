// What the mesh clean-up (mesh_components.hip), the mesh smoothing (mesh_smooth.hip) and the mesh simplification (mesh_simplify.hip) share: the
// sizes of a launch, the ranking of n counters in three launches, the in-place sort of a segment by one lane, the invalid-face protocol of a
// workspace's header, and on the host the argument checks and the table of remembered workspaces.  Include after common.h.
//
//   ranking      span_rank_kernel: a workgroup ranks a span of kSpan items (a wave scan of the threads' shares, LDS across the waves);
//                span_scan_kernel: ONE workgroup scans the spans' sums in 64 bits; the consumer adds its span's offset.  No look-back, no
//                grid barrier, nothing waits for another workgroup.  Ranks are integers: no result depends on which thread took which item.
//   header       the first kHeaderBytes of a workspace are int64 words; kHdrInvalid and kHdrFirstInvalid have the same place in every file.
//                The first launch that reads `faces` range-checks them (record_invalid_face), every later launch does nothing when the count
//                is not zero, and the entry point's one read-back refuses with the count and the lowest index (read_header).
#pragma once
#include "common.h"

#include <mutex>

namespace nm_mesh {

constexpr int kThreads = 256;                                 // every launch, the one-workgroup scan included
constexpr int kSpan = 1024;                                   // items (counters or flags) one workgroup of a ranking covers
constexpr int kPerThread = kSpan / kThreads;                  // consecutive items of one thread
constexpr int kSortInThread = 32;                             // a segment of up to this many entries: insertion sort; longer: heap sort
constexpr int64_t kHeaderBytes = 64;
static_assert(kSpan % kThreads == 0 && kThreads % 64 == 0, "a span is whole threads' shares, a workgroup whole waves");

enum { kHdrInvalid = 1, kHdrFirstInvalid = 2 };               // int64 words of every header; the other words are the file's own

// ---- header -----------------------------------------------------------------------------------------------------------------------------
static __global__ void reset_header_kernel(int64_t* __restrict__ hdr) {
    if (threadIdx.x < kHeaderBytes / 8) hdr[threadIdx.x] = threadIdx.x == kHdrFirstInvalid ? INT64_MAX : 0;
}

__device__ __forceinline__ bool in_range(int32_t i, int64_t n) { return i >= 0 && (int64_t)i < n; }

// face f names a vertex out of range: one more of them, and the lowest index among them
__device__ __forceinline__ void record_invalid_face(int64_t* hdr, int64_t f) {
    atomicAdd(reinterpret_cast<unsigned long long*>(hdr + kHdrInvalid), 1ull);
    atomicMin(reinterpret_cast<long long*>(hdr + kHdrFirstInvalid), (long long)f);
}

// ---- ranking ----------------------------------------------------------------------------------------------------------------------------
struct Counters {                                             // the plain source of a ranking: an array of counters
    const int32_t* c;
    __device__ int count(int64_t i) const { return c[i]; }
};

// Source: count(i) -> int, the counter of item i < n (a flag counts 0 or 1).  out[i] = the sum of the span's counters before i, span_sum[span]
// = the sum of the span's counters.  `out` may be the source's own array: a thread reads its items before it writes them.  mark_empty: a zero
// counter's entry reads -1 (a flag's rank is asked for only where the flag is set).  skip_if: null, or a word that stops the launch when not 0.
template <class Source>
__global__ void __launch_bounds__(kThreads) span_rank_kernel(Source src, int64_t n, int32_t* out, int mark_empty, int64_t* __restrict__ span_sum,
                                                             const int64_t* skip_if) {
    __shared__ int s_wave[kThreads / 64];
    if (skip_if && *skip_if != 0) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t first = (int64_t)blockIdx.x * kSpan + (int64_t)threadIdx.x * kPerThread;
    int c[kPerThread], mine = 0;
#pragma unroll
    for (int r = 0; r < kPerThread; ++r) {
        c[r] = first + r < n ? src.count(first + r) : 0;
        mine += c[r];
    }
    int incl = mine;                                           // inclusive scan of the threads' shares across the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) {
        const int m = s_wave[w];
        before += w < wave ? m : 0;
        total += m;
    }
    int run = before + incl - mine;
#pragma unroll
    for (int r = 0; r < kPerThread; ++r) {
        if (first + r < n) out[first + r] = (mark_empty && c[r] == 0) ? -1 : run;
        run += c[r];
    }
    if (threadIdx.x == 0) span_sum[blockIdx.x] = total;
}

// exclusive scan of the spans' sums by one workgroup, ceil(spans / kThreads) spans per thread: the total -> *total and, if given, *end (the
// callers' totals are below 2^31)
static __global__ void __launch_bounds__(kThreads) span_scan_kernel(const int64_t* __restrict__ span_sum, int64_t spans, int64_t* __restrict__ span_off,
                                                                    int64_t* total, int32_t* __restrict__ end, const int64_t* skip_if) {
    __shared__ int64_t part[kThreads];
    if (skip_if && *skip_if != 0) return;
    const int64_t per = (spans + kThreads - 1) / kThreads, lo = threadIdx.x * per, hi = lo + per < spans ? lo + per : spans;
    int64_t s = 0;
    for (int64_t i = lo; i < hi; ++i) s += span_sum[i];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t run = 0;
        for (int i = 0; i < kThreads; ++i) {
            const int64_t t = part[i];
            part[i] = run;
            run += t;
        }
        *total = run;
        if (end) *end = (int32_t)run;
    }
    __syncthreads();
    int64_t run = part[threadIdx.x];
    for (int64_t i = lo; i < hi; ++i) {
        span_off[i] = run;
        run += span_sum[i];
    }
}

// ---- sort -------------------------------------------------------------------------------------------------------------------------------
// ascending, in place, by one lane: insertion sort up to kSortInThread entries, heap sort beyond (O(k log k), no second buffer)
__device__ inline void sort_segment(int32_t* a, int n) {
    if (n <= kSortInThread) {
        for (int i = 1; i < n; ++i) {
            const int32_t x = a[i];
            int j = i;
            while (j > 0 && a[j - 1] > x) {
                a[j] = a[j - 1];
                --j;
            }
            a[j] = x;
        }
        return;
    }
    for (int start = n / 2 - 1, end = n; end > 1;) {          // heap construction (start counts down to 0), then n - 1 extractions
        int root;
        int32_t x;
        if (start >= 0) {
            root = start--;
            x = a[root];
        } else {
            --end;
            x = a[end];
            a[end] = a[0];
            root = 0;
        }
        while (true) {                                         // sift x down from the hole at root, inside [0, end)
            int child = 2 * root + 1;
            if (child >= end) break;
            int32_t cv = a[child];
            if (child + 1 < end) {
                const int32_t other = a[child + 1];
                if (other > cv) {
                    cv = other;
                    ++child;
                }
            }
            if (cv <= x) break;
            a[root] = cv;
            root = child;
        }
        a[root] = x;
    }
}

// ---- host: sizes and argument checks ----------------------------------------------------------------------------------------------------
inline int64_t up16(int64_t b) { return (b + 15) / 16 * 16; }
inline int64_t spans_of(int64_t n) { return (n + kSpan - 1) / kSpan; }
inline unsigned blocks_for(int64_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }

inline bool count_ok(int64_t n) { return n >= 0 && n < (1ll << 31); }
inline bool mesh_ok(int64_t V, int64_t F) { return count_ok(V) && F >= 0 && F < (1ll << 31) && count_ok(3 * F); }

// two byte ranges share a byte (a null pointer or an empty range shares nothing)
inline bool overlap(const void* a, int64_t a_bytes, const void* b, int64_t b_bytes) {
    if (!a || !b || a_bytes <= 0 || b_bytes <= 0) return false;
    const uintptr_t p = reinterpret_cast<uintptr_t>(a), q = reinterpret_cast<uintptr_t>(b);
    return p < q + (uintptr_t)b_bytes && q < p + (uintptr_t)a_bytes;
}

struct Range {
    const void* p;
    int64_t bytes;
};

// every range of `outs` against every other range of `outs` and every range of `ins`
inline bool any_overlap(const Range* outs, int n_outs, const Range* ins, int n_ins) {
    for (int i = 0; i < n_outs; ++i) {
        for (int j = i + 1; j < n_outs; ++j)
            if (overlap(outs[i].p, outs[i].bytes, outs[j].p, outs[j].bytes)) return true;
        for (int j = 0; j < n_ins; ++j)
            if (overlap(outs[i].p, outs[i].bytes, ins[j].p, ins[j].bytes)) return true;
    }
    return false;
}

// `workspace` and `workspace_bytes` are the entry point's arguments, `need` the bytes its layout asks for
#define NM_MESH_WORKSPACE(who, need)                                                                                                         \
    NM_REQUIRE(workspace, who ": null workspace");                                                                                           \
    NM_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, who ": workspace must be 16-byte aligned");                              \
    NM_REQUIRE(workspace_bytes >= (need), who ": workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)(need))

// the one read-back of an entry point that validates faces: the first `words` words of the header -> head, the stream synchronised, and the
// refusal when a face named a vertex outside [0, V)
inline int read_header(const char* who, const int64_t* hdr, int64_t* head, int words, int64_t V, hipStream_t st) {
    hipError_t e = hipMemcpyAsync(head, hdr, (size_t)words * 8, hipMemcpyDeviceToHost, st);
    if (e != hipSuccess) {
        nm::set_error("%s: read counts: %s", who, hipGetErrorString(e));
        return NM_ERR_HIP;
    }
    if ((e = hipStreamSynchronize(st)) != hipSuccess) {
        nm::set_error("%s: sync: %s", who, hipGetErrorString(e));
        return NM_ERR_HIP;
    }
    NM_REQUIRE(head[kHdrInvalid] == 0, "%s: %lld invalid faces (an index outside [0, %lld)), the first of them face %lld", who,
               (long long)head[kHdrInvalid], (long long)V, (long long)head[kHdrFirstInvalid]);
    return NM_OK;
}

// ---- host: remembered workspaces --------------------------------------------------------------------------------------------------------
// What a count entry point left in a workspace, remembered on the host by the workspace's address, so that the fill entry points can compare
// their counts without a read-back: the last kRemembered workspaces.  Record: an aggregate with a member `const void* workspace`.
constexpr int kRemembered = 64;

template <class Record>
class Remembered {
  public:
    void remember(const Record& r) {
        std::lock_guard<std::mutex> lock(mutex_);
        for (int i = 0; i < kRemembered; ++i)
            if (rows_[i].workspace == r.workspace) {
                rows_[i] = r;
                return;
            }
        rows_[next_] = r;
        next_ = (next_ + 1) % kRemembered;
    }
    void forget(const void* workspace) {
        std::lock_guard<std::mutex> lock(mutex_);
        for (int i = 0; i < kRemembered; ++i)
            if (rows_[i].workspace == workspace) rows_[i] = Record{};
    }
    bool recall(const void* workspace, Record* out) {
        std::lock_guard<std::mutex> lock(mutex_);
        for (int i = 0; i < kRemembered; ++i)
            if (rows_[i].workspace == workspace) {
                *out = rows_[i];
                return true;
            }
        return false;
    }

  private:
    std::mutex mutex_;
    Record rows_[kRemembered] = {};
    int next_ = 0;
};

}  // namespace nm_mesh
