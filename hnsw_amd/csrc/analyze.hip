// analyze.hip -- the Analyzer's device side (analyze_host.cpp): a layer's degree histogram, the
// reachability BFS from the searches' entry down the layers, and the multi-source hop BFS of the
// quality metrics.  None of them reads a vector: they walk `deg` and `adj` only.  Everything a
// caller can observe is integer work whose result does not depend on scheduling: histograms and
// popcounts are integer sums, a BFS level is a set, and the lists come from ordered compaction
// of a bitmap (rowset.hip).  A BFS level is one kernel launch (the hop BFS: two); the launch
// boundary is what makes a level's writes visible to the next, on every XCD -- no kernel here
// waits on another workgroup.
#include "block_scan.hpp"
#include "engine.hpp"

namespace mh {

// a stored neighbour id as a row to visit: negative entries are empty slots, ids at or past the
// allocated rows are reported (GraphDev::err bit 4) and skipped
__device__ __forceinline__ bool an_edge(int32_t x, uint32_t capn, int* err) {
    if (x < 0) return false;
    if ((uint32_t)x >= capn) {
        atomicOr(err, 4);
        return false;
    }
    return true;
}
__device__ __forceinline__ int an_deg(const int32_t* __restrict__ deg, int64_t row, int cap) {
    const int d = deg[row];
    return d < 0 ? 0 : (d > cap ? cap : d);
}

// ---- degree histogram of a layer's live members ----
// hist[d] += live members of degree d (a degree below 0 counts as 0, one past the last bin as
// the last bin: the host refuses layers whose rows can hold more).  Per-block LDS bins, then
// one integer atomic per non-empty bin and block.
__global__ __launch_bounds__(256) void k_an_degree(const int32_t* __restrict__ deg, const uint8_t* __restrict__ dead,
                                                   int64_t n, unsigned long long* __restrict__ hist) {
    __shared__ uint32_t bins[AN_BINS];
    for (int i = threadIdx.x; i < AN_BINS; i += 256) bins[i] = 0;
    __syncthreads();
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (int64_t)gridDim.x * 256) {
        const int d = deg[r];
        if (d == -2 || (dead && dead[r])) continue;
        atomicAdd(&bins[d < 0 ? 0 : (d >= AN_BINS ? AN_BINS - 1 : d)], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < AN_BINS; i += 256)
        if (bins[i]) atomicAdd(&hist[i], (unsigned long long)bins[i]);
}

int launch_an_degree(const int32_t* deg, const uint8_t* dead, int64_t n, unsigned long long* hist, hipStream_t s) {
    if (n <= 0) return 0;
    const int64_t grid = std::min<int64_t>((n + 255) / 256, 2048);
    hipLaunchKernelGGL(k_an_degree, dim3((unsigned)grid), dim3(256), 0, s, deg, dead, n, hist);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---- reachability ----
// lanes with `take` append v to q at one atomicAdd per wave: a ballot names them, its popcount
// is their number, a lane's rank among them its slot
__device__ __forceinline__ void an_append(bool take, uint32_t v, uint32_t* __restrict__ q, uint32_t* __restrict__ qcnt) {
    const unsigned long long m = __ballot(take);
    if (!m) return;
    const int lane = lane_id();
    uint32_t base = 0;
    if (lane == __ffsll((long long)m) - 1) base = atomicAdd(qcnt, (uint32_t)__popcll(m));
    base = shfl_u(base, __ffsll((long long)m) - 1);
    if (take) q[base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = v;
}

// The seeds of a layer below the top: the rows the layer above reached that are members here
// (deg != -2; deleted rows route).  vis &= membership, and every row left is queued.  One thread
// per row; a wave's 64 rows are the bitmap words 2w and 2w + 1 (vis holds an even word count).
__global__ __launch_bounds__(256) void k_an_seed(const int32_t* __restrict__ deg, int64_t n, int64_t rows,
                                                 uint32_t* __restrict__ vis, uint32_t* __restrict__ q,
                                                 uint32_t* __restrict__ qcnt) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r - lane_id() >= rows) return;  // (a whole wave)
    const bool member = r < n && deg[r] != -2;
    const unsigned long long m = __ballot(member);
    const int lane = lane_id();
    uint32_t w = 0;
    if ((lane & 31) == 0) {
        const uint32_t mb = lane ? (uint32_t)(m >> 32) : (uint32_t)m;
        w = vis[r >> 5] & mb;
        vis[r >> 5] = w;
    }
    w = shfl_u(w, lane & 32);
    an_append((w >> (lane & 31)) & 1u, (uint32_t)r, q, qcnt);
}

// One BFS level, one wave per frontier row: lane j takes the row's j-th neighbour.  The value
// atomicOr returns alone decides who found a row first (the plain read before it only spares
// the atomic for rows already seen: bits are never cleared during a level, so a stale read
// errs towards doing the atomic).
__global__ __launch_bounds__(256) void k_an_level(const int32_t* __restrict__ deg, const int32_t* __restrict__ adj,
                                                  int cap, uint32_t capn, const uint32_t* __restrict__ cur,
                                                  uint32_t ncur, uint32_t* __restrict__ vis,
                                                  uint32_t* __restrict__ next, uint32_t* __restrict__ ncnt,
                                                  int* __restrict__ err) {
    const int64_t wv = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wv >= (int64_t)ncur) return;
    const uint32_t row = cur[wv];
    const int lane = lane_id();
    const int d = an_deg(deg, row, cap);
    for (int j0 = 0; j0 < d; j0 += 64) {
        const int j = j0 + lane;
        bool fresh = false;
        uint32_t v = 0;
        if (j < d) {
            const int32_t x = adj[(size_t)row * cap + j];
            if (an_edge(x, capn, err)) {
                v = (uint32_t)x;
                const uint32_t bit = 1u << (v & 31);
                if (!(vis[v >> 5] & bit)) fresh = !(atomicOr(&vis[v >> 5], bit) & bit);
            }
        }
        an_append(fresh, v, next, ncnt);
    }
}

// A layer's counts from its final bitmap: cnt[0] += live members (deg != -2, not deleted),
// cnt[1] += those visited; unr (nullable): the live members not visited, as bitmap words.
__global__ __launch_bounds__(256) void k_an_count(const int32_t* __restrict__ deg, const uint8_t* __restrict__ dead,
                                                  int64_t n, int64_t rows, const uint32_t* __restrict__ vis,
                                                  uint32_t* __restrict__ unr, unsigned long long* __restrict__ cnt) {
    __shared__ uint32_t part[2][8];
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const bool live = r < n && deg[r] != -2 && !(dead && dead[r]);
    const unsigned long long m = __ballot(live);
    if ((lane & 31) == 0) {
        uint32_t mem = 0, hit = 0;
        if (r < rows) {
            const uint32_t mb = lane ? (uint32_t)(m >> 32) : (uint32_t)m;
            const uint32_t v = vis[r >> 5];
            if (unr) unr[r >> 5] = mb & ~v;
            mem = (uint32_t)__popc(mb);
            hit = (uint32_t)__popc(mb & v);
        }
        part[0][wave * 2 + (lane >> 5)] = mem;
        part[1][wave * 2 + (lane >> 5)] = hit;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        uint32_t t = 0;
        for (int i = 0; i < 8; ++i) t += part[threadIdx.x][i];
        if (t) atomicAdd(&cnt[threadIdx.x], (unsigned long long)t);
    }
}

// `rows`: the bitmap's rows, a multiple of 64 at or past capn
int launch_an_seed(const int32_t* deg, int64_t n, int64_t rows, uint32_t* vis, uint32_t* q, uint32_t* qcnt,
                   hipStream_t s) {
    if (rows <= 0) return 0;
    hipLaunchKernelGGL(k_an_seed, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, deg, n, rows, vis, q, qcnt);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int launch_an_level(const int32_t* deg, const int32_t* adj, int cap, uint32_t capn, const uint32_t* cur, uint32_t ncur,
                    uint32_t* vis, uint32_t* next, uint32_t* ncnt, int* err, hipStream_t s) {
    if (ncur == 0) return 0;
    hipLaunchKernelGGL(k_an_level, dim3((ncur + 3) / 4), dim3(256), 0, s, deg, adj, cap, capn, cur, ncur, vis, next, ncnt,
                       err);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int launch_an_count(const int32_t* deg, const uint8_t* dead, int64_t n, int64_t rows, const uint32_t* vis, uint32_t* unr,
                    unsigned long long* cnt, hipStream_t s) {
    if (rows <= 0) return 0;
    hipLaunchKernelGGL(k_an_count, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, deg, dead, n, rows, vis, unr,
                       cnt);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

__global__ void k_an_keys(const int64_t* __restrict__ keys, const uint32_t* __restrict__ ids, int64_t m,
                          int64_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m) out[i] = keys[ids[i]];
}
int launch_an_keys(const int64_t* keys, const uint32_t* ids, int64_t m, int64_t* out, hipStream_t s) {
    if (m <= 0) return 0;
    hipLaunchKernelGGL(k_an_keys, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, keys, ids, m, out);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---- multi-source hop BFS ----
// A row's state is three 128-bit masks, bit i for source i: seen, cur (the frontier) and next.
// src[i] is source i's row; sidx[row] = i for those rows, -1 elsewhere (the host fills it).
__global__ void k_an_hops_init(const uint32_t* __restrict__ src, int ns, uint32_t* __restrict__ seen,
                               uint32_t* __restrict__ cur, int32_t* __restrict__ sidx) {
    const int i = threadIdx.x;
    if (i >= ns) return;
    const uint32_t row = src[i];
    seen[(size_t)row * 4 + (i >> 5)] = 1u << (i & 31);  // (the sources are distinct rows)
    cur[(size_t)row * 4 + (i >> 5)] = 1u << (i & 31);
    sidx[row] = i;
}

// push, one wave per row of the frontier: cur is ORed into next of every neighbour, by 32-bit
// atomicOr and only on words that add a bit the neighbour has not seen (seen is not written
// during this launch; the read of next only spares atomics)
__global__ __launch_bounds__(256) void k_an_hops_push(const int32_t* __restrict__ deg, const int32_t* __restrict__ adj,
                                                      int cap, uint32_t capn, int64_t n, const uint32_t* __restrict__ seen,
                                                      const uint32_t* __restrict__ cur, uint32_t* __restrict__ next,
                                                      int* __restrict__ err) {
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const uint4 c4 = *reinterpret_cast<const uint4*>(cur + (size_t)row * 4);
    if (!(c4.x | c4.y | c4.z | c4.w)) return;
    const uint32_t c[4] = {c4.x, c4.y, c4.z, c4.w};
    const int lane = lane_id();
    const int d = an_deg(deg, row, cap);
    for (int j = lane; j < d; j += 64) {
        const int32_t x = adj[(size_t)row * cap + j];
        if (!an_edge(x, capn, err)) continue;
        const uint4 s4 = *reinterpret_cast<const uint4*>(seen + (size_t)x * 4);
        const uint32_t sv[4] = {s4.x, s4.y, s4.z, s4.w};
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const uint32_t add = c[w] & ~sv[w];
            if (add && (add & ~next[(size_t)x * 4 + w])) atomicOr(&next[(size_t)x * 4 + w], add);
        }
    }
}

// settle, one thread per row: new = next & ~seen joins seen and becomes the frontier, next is
// cleared; a source row records the level for every source that reached it now; *any is set
// when some frontier is left
__global__ __launch_bounds__(256) void k_an_hops_settle(int64_t rows, uint32_t* __restrict__ seen,
                                                        uint32_t* __restrict__ cur, uint32_t* __restrict__ next,
                                                        const int32_t* __restrict__ sidx, int ns, int level,
                                                        int32_t* __restrict__ hops, uint32_t* __restrict__ any) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool left = false;
    if (r < rows) {
        const uint4 n4 = *reinterpret_cast<const uint4*>(next + (size_t)r * 4);
        const uint4 c4 = *reinterpret_cast<const uint4*>(cur + (size_t)r * 4);
        if (n4.x | n4.y | n4.z | n4.w) {
            uint4 s4 = *reinterpret_cast<const uint4*>(seen + (size_t)r * 4);
            const uint32_t nw[4] = {n4.x & ~s4.x, n4.y & ~s4.y, n4.z & ~s4.z, n4.w & ~s4.w};
            s4.x |= nw[0], s4.y |= nw[1], s4.z |= nw[2], s4.w |= nw[3];
            *reinterpret_cast<uint4*>(seen + (size_t)r * 4) = s4;
            *reinterpret_cast<uint4*>(cur + (size_t)r * 4) = make_uint4(nw[0], nw[1], nw[2], nw[3]);
            *reinterpret_cast<uint4*>(next + (size_t)r * 4) = make_uint4(0u, 0u, 0u, 0u);
            left = (nw[0] | nw[1] | nw[2] | nw[3]) != 0;
            const int j = sidx[r];
            if (left && j >= 0)
                for (int w = 0; w < 4; ++w)
                    for (uint32_t b = nw[w]; b; b &= b - 1) {
                        const int i = w * 32 + __ffs((int)b) - 1;
                        if (i < ns) hops[(size_t)i * ns + j] = level;
                    }
        } else if (c4.x | c4.y | c4.z | c4.w) {
            *reinterpret_cast<uint4*>(cur + (size_t)r * 4) = make_uint4(0u, 0u, 0u, 0u);
        }
    }
    if (__ballot(left) && lane_id() == 0) atomicOr(any, 1u);
}

int launch_an_hops_init(const uint32_t* src, int ns, uint32_t* seen, uint32_t* cur, int32_t* sidx, hipStream_t s) {
    if (ns <= 0 || ns > AN_MAX_KEYS) return -1;
    hipLaunchKernelGGL(k_an_hops_init, dim3(1), dim3(AN_MAX_KEYS), 0, s, src, ns, seen, cur, sidx);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int launch_an_hops_push(const int32_t* deg, const int32_t* adj, int cap, uint32_t capn, int64_t n, const uint32_t* seen,
                        const uint32_t* cur, uint32_t* next, int* err, hipStream_t s) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_an_hops_push, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, deg, adj, cap, capn, n, seen, cur,
                       next, err);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int launch_an_hops_settle(int64_t rows, uint32_t* seen, uint32_t* cur, uint32_t* next, const int32_t* sidx, int ns,
                          int level, int32_t* hops, uint32_t* any, hipStream_t s) {
    if (rows <= 0) return 0;
    hipLaunchKernelGGL(k_an_hops_settle, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, rows, seen, cur, next,
                       sidx, ns, level, hops, any);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace mh
