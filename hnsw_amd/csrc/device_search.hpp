// device_search.hpp -- per-wave layer searches shared by the search kernels
// (search.hip) and the build kernels (build_compat.hpp, build_batch.hpp).
//
//   beam_layer   : sorted-list best-first search (standard HNSW Alg. 2 stop
//                  rule), restated in oracle/oracle.c beam_layer_search.
//   compat_layer : graph.go:94-170 layerNode.search with the reference's heap
//                  quirks (Max()/PopLast() act on the last array slot, result
//                  in heap order, greedy stop), restated in oracle/oracle.c
//                  compat_layer_search.
#pragma once
#include "device_common.hpp"

namespace mh {

// Loads of mutable graph state.  COH = true inside the sequential build /
// delete kernels, which rewrite adjacency while searching: relaxed atomics
// keep the compiler off the (incoherent) scalar cache.  Only one wave ever
// reads or writes graph state there (the multi-wave build's workers score
// immutable rows), so wavefront scope suffices -- and it keeps the loads in
// the vector L1 (workgroup scope would add sc0, sending every dependent load
// of the walk to L2); the wave's own program order and __syncthreads /
// ev.sync() order its lanes.
// The pointers come from the layer table, so the compiler cannot tell their
// address space: the casts make these global (not flat) operations, which do
// not count against lgkmcnt (a flat load holds up every LDS wait behind it).
typedef __attribute__((address_space(1))) int32_t g_i32;
template <bool COH>
__device__ __forceinline__ int32_t ld_i32(const int32_t* p) {
    const g_i32* gp = (const g_i32*)p;
    if constexpr (COH)
        return __hip_atomic_load(gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    else
        return *gp;
}
__device__ __forceinline__ void st_i32(int32_t* p, int32_t v) {
    __hip_atomic_store((g_i32*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}

// `layers[l].nodes[*elevator]` (graph.go:497, 574): the layer's node of the
// elevator row's KEY -- the key's live row that is a member of layer l (its
// newest, then the older ones through kprev), else nil (EMPTY_ID).  The
// elevator itself may be a replaced or deleted node that a dangling edge led to.
template <bool COH>
__device__ __forceinline__ uint32_t resolve_member(const GraphDev& g, int l, uint32_t e) {
    if (g.kidlive) {
        int32_t r = ld_i32<COH>(g.kidlive + kid_of(g, e));
        for (int hop = 0; hop < MH_MAXL && r >= 0 && (uint32_t)r < g.capn; ++hop) {  // (rows hold disjoint layers)
            if (ld_i32<COH>(g.layers[l].deg + r) != -2 && !is_dead(g, (uint32_t)r)) return (uint32_t)r;
            r = g.kprev ? ld_i32<COH>(g.kprev + r) : -1;
        }
        return EMPTY_ID;
    }
    if (e >= g.capn || ld_i32<COH>(g.layers[l].deg + e) == -2 || is_dead(g, e)) return EMPTY_ID;
    return e;
}

// Evaluate the distances of candidate ids held in lanes 0..cnt-1 of `cid`
// against the query; sink(dist, id) is called in row order (uniformly).
template <class C, int G, class Sink>
__device__ __forceinline__ void eval_list(const GraphDev& g, const QReg<C>& q, float qn, uint32_t cid, int cnt,
                                          int metric, Sink&& sink) {
    using RM = RowMap<C, G>;
    const int lane = lane_id();
    for (int base = 0; base < cnt; base += RM::T) {
        uint32_t ids[G];
        bool valid[G];
#pragma unroll
        for (int gg = 0; gg < G; ++gg) {
            const int t = base + RM::reg_row(gg, lane);
            valid[gg] = t < cnt;
            if constexpr (C::RPI == 1)
                ids[gg] = rl_u(cid, (base + gg) & 63);
            else
                ids[gg] = shfl_u(cid, t & 63);
            ids[gg] = valid[gg] ? guard_id(g, ids[gg]) : 0u;
        }
        float s;
        if (metric == EUCLIDEAN)
            s = eval_rows<C, G, true>(q, g.vecs, g.pitch, ids, valid);
        else
            s = eval_rows<C, G, false>(q, g.vecs, g.pitch, ids, valid);
        const int town = base + RM::owned_row(lane);
        const uint32_t idown = shfl_u(cid, town & 63);
        float xn = 1.f;
        if (metric == COSINE && town < cnt) xn = g.norms[guard_id(g, idown)];
        const float dist = finalize(metric, s, xn, qn);
#pragma unroll
        for (int t = 0; t < RM::T; ++t) {
            if (base + t >= cnt) break;
            sink(rl_f(dist, RM::owner(t)), rl_u(cid, (base + t) & 63));
        }
    }
}

// compact the lanes where `keep` holds into lanes 0..popc-1 (order preserving)
__device__ __forceinline__ uint32_t compact(uint32_t v, bool keep, int& cnt) {
    const unsigned long long m = __ballot(keep);
    cnt = __popcll(m);
    const int lane = lane_id();
    const int before = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0));
    const int dst = keep ? before : cnt + (lane - before);
    return push_to(v, dst);
}

// Screened evaluation for the sorted-list searches: candidates whose fp16
// screening distance proves the f32 distance exceeds `wd` (the list's worst
// entry before this batch, which only decreases) are dropped; the rest go
// through eval_list, so every distance that reaches the sink is the canonical
// f32 one and the list evolves exactly as without the screen.
// Returns the number of rows evaluated in f32.
template <class C, int G, class Sink>
__device__ __forceinline__ int eval_screened(const GraphDev& g, const QReg<C>& q, float qn, uint32_t cid, int cnt,
                                             int metric, float wd, Sink&& sink, unsigned long long& s16,
                                             float margin) {
    constexpr int GH = (2 * G <= C::LPR) ? 2 * G : G;
    using RM = RowMap<C, GH>;
    const int lane = lane_id();
    if (!g.h16) {
        eval_list<C, G>(g, q, qn, cid, cnt, metric, sink);
        return cnt;
    }
    s16 += cnt;
    bool rej = false;  // lane t: candidate t is rejected
    for (int base = 0; base < cnt; base += RM::T) {
        uint32_t ids[GH];
        bool valid[GH];
        float inv[GH];
#pragma unroll
        for (int gg = 0; gg < GH; ++gg) {
            const int t = base + RM::reg_row(gg, lane);
            valid[gg] = t < cnt;
            if constexpr (C::RPI == 1)
                ids[gg] = rl_u(cid, (base + gg) & 63);
            else
                ids[gg] = shfl_u(cid, t & 63);
            ids[gg] = valid[gg] ? guard_id(g, ids[gg]) : 0u;
        }
        const int town = base + RM::owned_row(lane);
        bool r = false;
        if (metric == EUCLIDEAN) {
            float xn[GH];
#pragma unroll
            for (int gg = 0; gg < GH; ++gg) {
                const float2 ax = g.h16aux[ids[gg]];
                inv[gg] = ax.x;
                xn[gg] = ax.y;
            }
            const float s = eval_rows_h16<C, GH, true>(q, g.h16, g.pitch, ids, valid, inv);
            // the owner of row town computed it in register (town - base) / RPI
            float xo = xn[0];
#pragma unroll
            for (int gg = 1; gg < GH; ++gg)
                if (RM::reg_row(gg, lane) == town - base) xo = xn[gg];
            if (town < cnt) r = h16_rejects_l2(s, xo, wd, margin);
        } else {
#pragma unroll
            for (int gg = 0; gg < GH; ++gg) inv[gg] = 1.f;
            const float s = eval_rows_h16<C, GH, false>(q, g.h16, g.pitch, ids, valid, inv);
            if (town < cnt) r = h16_rejects_cos(s, qn, wd, margin);
        }
        // hand row t's verdict from its owner lane to lane t
        const int t = lane - base;
        const int src = (t >= 0 && t < RM::T) ? RM::owner(t) : lane;
        const bool rt = __shfl((int)r, src, 64) != 0;
        if (t >= 0 && t < RM::T) rej = rt;
    }
    int cnt2;
    const uint32_t cid2 = compact(cid, lane < cnt && !rej, cnt2);
    if (cnt2 > 0) eval_list<C, G>(g, q, qn, cid2, cnt2, metric, sink);
    return cnt2;
}

// Two-sided screen of the rows cid[0, cnt) against a stored row held as the
// "query" q (norm qn), for the selection rule "r drops c when alpha d(c, r) <
// d(u, c)": lane t gets +1 when row t's f32 distance is certainly > hi_t, -1
// when it is certainly < lo_t, 0 when the fp16 estimate cannot tell (those go
// to the canonical f32 path).  lo_t / hi_t: row t's bounds, in lane t (or the
// same in every lane).  Rows outside the copy's range are always 0.
template <class C, int G>
__device__ __forceinline__ int screen_pairs(const GraphDev& g, const QReg<C>& q, float qn, uint32_t cid, int cnt,
                                            int metric, float lo_t, float hi_t, float margin) {
    constexpr int GH = (2 * G <= C::LPR) ? 2 * G : G;
    using RM = RowMap<C, GH>;
    const int lane = lane_id();
    int cls = 0;
    for (int base = 0; base < cnt; base += RM::T) {
        uint32_t ids[GH];
        bool valid[GH];
        float inv[GH];
#pragma unroll
        for (int gg = 0; gg < GH; ++gg) {
            const int t = base + RM::reg_row(gg, lane);
            valid[gg] = t < cnt;
            if constexpr (C::RPI == 1)
                ids[gg] = rl_u(cid, (base + gg) & 63);
            else
                ids[gg] = shfl_u(cid, t & 63);
            ids[gg] = valid[gg] ? guard_id(g, ids[gg]) : 0u;
        }
        const int town = base + RM::owned_row(lane);
        const float lo = __shfl(lo_t, town & 63, 64), hi = __shfl(hi_t, town & 63, 64);
        int c = 0;
        if (metric == EUCLIDEAN) {
            float xn[GH];
#pragma unroll
            for (int gg = 0; gg < GH; ++gg) {
                const float2 ax = g.h16aux[ids[gg]];
                inv[gg] = ax.x;
                xn[gg] = ax.y;
            }
            const float s = eval_rows_h16<C, GH, true>(q, g.h16, g.pitch, ids, valid, inv);
            float xo = xn[0];
#pragma unroll
            for (int gg = 1; gg < GH; ++gg)
                if (RM::reg_row(gg, lane) == town - base) xo = xn[gg];
            if (town < cnt) c = h16_rejects_l2(s, xo, hi, margin) ? 1 : h16_below_l2(s, xo, lo, margin) ? -1 : 0;
        } else {
#pragma unroll
            for (int gg = 0; gg < GH; ++gg) inv[gg] = 1.f;
            const float s = eval_rows_h16<C, GH, false>(q, g.h16, g.pitch, ids, valid, inv);
            if (town < cnt) c = h16_rejects_cos(s, qn, hi, margin) ? 1 : h16_below_cos(s, qn, lo, margin) ? -1 : 0;
        }
        const int t = lane - base;
        const int src = (t >= 0 && t < RM::T) ? RM::owner(t) : lane;
        const int ct = __shfl(c, src, 64);
        if (t >= 0 && t < RM::T) cls = ct;
    }
    return cls;
}

struct WaveStats {
    unsigned long long E = 0, X = 0, resets = 0;
    unsigned long long S = 0, F = 0;  // rows screened on the fp16 copy / rows evaluated in f32
#ifdef MH_PROF_BEAM
    // (tools-only build, tools/Makefile.beam: shader-clock cycles of the layer-0
    // beam spent in list insertions, in candidate scoring, and in all)
    unsigned long long c_ins = 0, c_score = 0, c_all = 0;
#endif
};

// Orders the lanes of ONE wave (compiler ordering only: a wave's vector memory
// and LDS operations are performed in issue order, so a lane's load after
// another lane's store to the same address sees it -- no waitcnt for the
// store's acknowledgement).  The sequential walks mutate graph state from a
// single wave; nothing else reads it while they run.
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// How the sequential (compat) walks evaluate distances and order their own
// lanes.  WaveEval: everything on the calling wave (a 64-thread workgroup, so
// __syncthreads only orders this wave).  The multi-wave build evaluator
// (build_compat.hpp MwEval) has the same interface and spreads each batch of rows
// over the workgroup's other waves.
struct WaveEval {
    static constexpr bool kPairs = false;  // no batched per-row scoring (build_compat.hpp MwEval::pairs)
    uint32_t* list = nullptr;  // LDS candidate list (run_list)
    template <class C, int G, class Sink>
    __device__ __forceinline__ void run(const GraphDev& g, const QReg<C>& q, float qn, uint32_t cid, int cnt,
                                        int metric, Sink&& sink) const {
        eval_list<C, G>(g, q, qn, cid, cnt, metric, sink);
    }
    // rows list[0, cnt), sink called in list order
    template <class C, int G, class Sink>
    __device__ __forceinline__ void run_list(const GraphDev& g, const QReg<C>& q, float qn, int cnt, int metric,
                                             Sink&& sink) const {
        for (int b = 0; b < cnt; b += 64) {
            const int c = min(64, cnt - b);
            const uint32_t cid = lane_id() < c ? list[b + lane_id()] : 0u;
            eval_list<C, G>(g, q, qn, cid, c, metric, sink);
        }
    }
    // rows list[0, cnt): distance e into outd[e], the row into outi[e]
    template <class C, int G>
    __device__ __forceinline__ void score(const GraphDev& g, const QReg<C>& q, float qn, int cnt, int metric,
                                          float* outd, uint32_t* outi) const {
        int t = 0;
        run_list<C, G>(g, q, qn, cnt, metric, [&](float d, uint32_t u) {
            if (lane_id() == 0) {
                outd[t] = d;
                outi[t] = u;
            }
            ++t;
        });
    }
    __device__ __forceinline__ void sync() const { wave_sync(); }
};

// the visited set's fill at which beam_layer forgets (3/4; a tools build may
// set another fraction to measure the probe-length / re-evaluation trade)
// beam_layer's visited set: vsize > 0 the 32-bit set of vsize entries, vsize < 0
// the compact 16-bit set (device_common.hpp VIS16_*; the query searches, ids < 2^24)
__device__ __forceinline__ int vis_any_probe(uint32_t* vis, int vsize, uint32_t id) {
    return vsize < 0 ? vis16_probe(vis, id) : vis_probe_n(vis, (uint32_t)vsize, id);
}
__device__ __forceinline__ void vis_any_clear(uint32_t* vis, int vsize) { vis_clear(vis, vsize < 0 ? VIS16_WORDS : vsize); }
__device__ __forceinline__ int vis_any_cap(int vsize) { return vsize < 0 ? VIS16_HOMES : vsize; }

#ifndef MH_VIS_FULL
#define MH_VIS_FULL(n) (((n) >> 1) + ((n) >> 2))
#endif

// Batched list update (the query search's 256- and 512-entry lists, beam_layer
// MERGE): a step's candidates that beat the list's worst entry are collected,
// one per lane, and merged into the list once per step instead of one
// bl_insert each.  bl_insert keeps the best ef of the list and everything
// offered to it, whatever the order (it drops a candidate only when it is no
// better than the worst entry or already listed), so the merge leaves the list
// bl_insert would, expansion marks included.  Fast path, every distance finite
// and distinct: each candidate ranked among the candidates (one compare per
// candidate) and in the list (binary search over the list's distances in LDS,
// A), every list entry moved down by the candidates ranked at or before it,
// and both written into A at their new places and read back (distances, then
// ids).  A candidate whose distance equals a listed one (the same row met
// again, or equal rows), any infinite distance, or a candidate that is worse
// than every listed entry (it beat the worst entry before the step, and an
// earlier flush of the same step lowered that) sends the buffer through
// bl_insert instead.  LDS scratch M: A = M[0, 512) (the list), the k <= 64
// candidates in M[512 + j] (distance) and M[576 + j] (id), in arrival order.
constexpr int BL_MERGE_WORDS = 640;
template <int R>
__device__ __forceinline__ void bl_merge(BList<R>& L, int ef, int k, float* M) {
    const int lane = lane_id();
    const float INF = __int_as_float(0x7f800000);
    float* A = M;
    wave_sync();  // (the buffer was written by lane 0)
    const float bd = lane < k ? M[512 + lane] : INF;
    const uint32_t bi = lane < k ? reinterpret_cast<const uint32_t*>(M)[576 + lane] : EMPTY_ID;
    const float d = bd;
    const uint32_t id = bi;
    bool slow = __ballot(lane < k && !(bd < INF)) != 0;
    int rk = 0;  // lane j < k: the candidates below candidate j
    int lb = 0;  // lane j < k: the list entries (of the first ef) below candidate j
    if (!slow) {
        int eq = 0;
        for (int j = 0; j < k; ++j) {
            const float dj = rl_f(bd, j);
            rk += dj < bd ? 1 : 0;
            eq += dj == bd ? 1 : 0;
        }
        slow = __ballot(lane < k && eq > 1) != 0;
    }
    if (!slow) {
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (r * 64 + lane < ef) A[r * 64 + lane] = L.d[r];
        wave_sync();
        if (lane < k) {
            // lower bound over A[0, ef], so that lb can reach ef: a candidate beat the
            // worst entry before the step, but a step's earlier flush (XW > 1, bk + cnt
            // > 64) may have lowered the worst entry below it.  Such a candidate must be
            // dropped, not placed on the last entry: lb == ef sends the buffer through
            // bl_insert, which drops it.  (The steps add up to 128 R - 1 >= ef; from
            // R * 32 they stopped at 64 R - 1 and never compared A[ef - 1] at ef = 64 R.)
#pragma unroll
            for (int step = R * 64; step >= 1; step >>= 1) {
                const int t = lb + step - 1;
                if (t < ef && A[t] < d) lb += step;
            }
        }
        slow = __ballot(lane < k && (lb >= ef || A[lb] == d)) != 0;
        wave_sync();
    }
    if (slow) {
        for (int j = 0; j < k; ++j) bl_insert(L, ef, rl_f(bd, j), rl_u(bi, j));
        return;
    }
    int sh[R];
#pragma unroll
    for (int r = 0; r < R; ++r) sh[r] = 0;
    for (int j = 0; j < k; ++j) {
        const int lj = rl_i(lb, j);
#pragma unroll
        for (int r = 0; r < R; ++r) sh[r] += (r * 64 + lane >= lj) ? 1 : 0;
    }
    const int pos = rk + lb;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int i = r * 64 + lane;
        if (i < ef && i + sh[r] < ef) A[i + sh[r]] = L.d[r];
    }
    if (lane < k && pos < ef) A[pos] = d;
    wave_sync();
#pragma unroll
    for (int r = 0; r < R; ++r)
        if (r * 64 + lane < ef) L.d[r] = A[r * 64 + lane];
    wave_sync();
    uint32_t* AI = reinterpret_cast<uint32_t*>(A);
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int i = r * 64 + lane;
        if (i < ef && i + sh[r] < ef) AI[i + sh[r]] = L.i[r];
    }
    if (lane < k && pos < ef) AI[pos] = id;
    wave_sync();
#pragma unroll
    for (int r = 0; r < R; ++r)
        if (r * 64 + lane < ef) L.i[r] = AI[r * 64 + lane];
    wave_sync();
}

// where beam_layer's MERGE steps buffer their candidates: distances in
// buf[0, 64), ids in buf[64, 128), in arrival order
template <int R>
__device__ __forceinline__ float* bl_cbuf(BList<R>&, float* mrg) {
    return mrg + 512;
}

// after a visited reset the list's members stay visited: they are the
// neighbourhood the next expansions keep meeting (fewer re-evaluations).
// Returns the ids recorded.
template <int R>
__device__ __forceinline__ int bl_seed(const BList<R>& L, uint32_t* vis, int vsize) {
    int seeded = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const uint32_t id = L.i[r];
        const bool ins = id != EMPTY_ID && vis_any_probe(vis, vsize, id & ID_MASK) == 1;
        seeded += __popcll(__ballot(ins));
    }
    return seeded;
}

// ---------------------------------------------------------------------------
// LDS-resident sorted list: the query search's layer 0 past the widest
// register list (512 < max(ef, k) <= LL_MAX_EF; option beam_lds_min_ef lowers
// the threshold).  The same list as BList -- entry i holds (d, id | EXP_BIT),
// ordered by (d, id), +inf / EMPTY_ID when empty -- with the same operations
// (bl_init / bl_at / bl_insert / bl_next / bl_merge / bl_seed), so beam_layer
// runs the same search on either.  All fields are wave-uniform.
//   n  : the filled entries, [0, n); the rest of [0, cap) is empty
//   nx : every entry below nx is expanded (bl_next scans from there)
// ---------------------------------------------------------------------------
constexpr int LL_MAX_EF = 2048;
struct LList {
    float* d;     // [cap] distances (LDS)
    uint32_t* i;  // [cap] ids
    float* cb;    // [128] the step's candidate buffer (bl_cbuf)
    int cap;      // a multiple of 64, >= ef
    int n, nx;
};
// the list's LDS words for max(ef, k) = efl: distances, ids, candidate buffer
__host__ __device__ inline int ll_cap(int efl) { return (efl + 63) & ~63; }
__host__ __device__ inline int ll_words(int efl) { return 2 * ll_cap(efl) + 128; }
__device__ __forceinline__ void ll_place(LList& L, uint32_t* mem, int efl) {
    L.cap = ll_cap(efl);
    L.cb = reinterpret_cast<float*>(mem);
    L.d = reinterpret_cast<float*>(mem + 128);
    L.i = mem + 128 + L.cap;
    L.n = L.nx = 0;
}

__device__ __forceinline__ float* bl_cbuf(LList& L, float*) { return L.cb; }

__device__ __forceinline__ void bl_init(LList& L) {
    for (int t = lane_id(); t < L.cap; t += 64) {
        L.d[t] = __int_as_float(0x7f800000);
        L.i[t] = EMPTY_ID;
    }
    L.n = L.nx = 0;
    wave_sync();
}

__device__ __forceinline__ void bl_at(const LList& L, int idx, float& d, uint32_t& id) {
    d = __int_as_float(uni(__float_as_int(L.d[idx])));
    id = uni(L.i[idx]);
}

// bl_insert's semantics (the best ef of the list and everything offered; NaN,
// a row already listed and anything no better than a full list's worst entry
// are dropped); entries [pos, n) move up by one, highest 64-entry chunk first.
__device__ __forceinline__ bool bl_insert(LList& L, int ef, float d, uint32_t u) {
    if (!(d == d)) return false;  // NaN never enters the list
    const int lane = lane_id();
    const int n = L.n;
    float wd;
    uint32_t wi;
    bl_at(L, ef - 1, wd, wi);
    if (!lt_di(d, u, wd, wi & ID_MASK)) return false;
    bool dup = false;
    int pos = 0;
    for (int b = 0; b < n; b += 64) {
        const int idx = b + lane;
        const bool in = idx < n;
        const float ed = in ? L.d[idx] : 0.f;
        const uint32_t ei = in ? L.i[idx] & ID_MASK : 0u;
        dup |= in && ei == u;
        pos += __popcll(__ballot(in && lt_di(ed, ei, d, u)));
    }
    if (__ballot(dup)) return false;
    for (int c = (n - 1) >> 6; c >= 0 && c * 64 + 63 >= pos; --c) {
        const int idx = c * 64 + lane;
        const bool mv = idx >= pos && idx < n && idx + 1 < ef;
        const float ed = mv ? L.d[idx] : 0.f;
        const uint32_t ei = mv ? L.i[idx] : 0u;
        wave_sync();  // (the chunk is read before its first entries are overwritten)
        if (mv) {
            L.d[idx + 1] = ed;
            L.i[idx + 1] = ei;
        }
        wave_sync();
    }
    if (lane == 0) {  // pos <= n, and pos < ef where the list is full (d beat its worst)
        L.d[pos] = d;
        L.i[pos] = u;
    }
    wave_sync();
    L.n = min(n + 1, ef);
    if (pos <= L.nx) L.nx = pos;
    return true;
}

// pick the first unexpanded entry, mark it expanded; returns EMPTY_ID if none
__device__ __forceinline__ uint32_t bl_next(LList& L) {
    const int lane = lane_id();
    for (int b = L.nx & ~63; b < L.n; b += 64) {
        const int idx = b + lane;
        const bool in = idx >= L.nx && idx < L.n;
        const uint32_t w = in ? L.i[idx] : EXP_BIT;
        const unsigned long long m = __ballot((w & EXP_BIT) == 0);
        if (m) {
            const int l = __ffsll((long long)m) - 1;
            const uint32_t id = rl_u(w, l);
            if (lane == l) L.i[idx] = w | EXP_BIT;
            wave_sync();
            L.nx = b + l + 1;
            return id;
        }
    }
    L.nx = L.n;
    return EMPTY_ID;
}

// the distance of the entry the last bl_next picked (it returned that entry's id)
__device__ __forceinline__ float bl_picked_dist(const LList& L) {
    return __int_as_float(uni(__float_as_int(L.d[L.nx - 1])));
}

// bl_merge over the LDS list: the k <= 64 candidates of L.cb, each ranked among
// the candidates and (binary search over L.d[0, ef], which can reach ef: see
// bl_merge) in the list.  The list's entries move up in place by the number of
// candidates placed at or before them (at most k <= 64 places), in 64-entry
// chunks from the tail down to the lowest insertion point: a chunk is read
// whole into registers before it is written, its writes go to indices at or
// above their sources, and every chunk above it has been read already, so
// nothing unread is overwritten and no second copy of the list is needed.
// The candidates are written last, into the places the shift left.
// An infinite distance, two equal candidate distances, a candidate equal to a
// listed distance and a candidate past every listed entry (lb >= ef) send the
// buffer through bl_insert, one candidate at a time.
__device__ __forceinline__ void bl_merge(LList& L, int ef, int k, float*) {
    const int lane = lane_id();
    const float INF = __int_as_float(0x7f800000);
    wave_sync();  // (the buffer was written by lane 0)
    const float bd = lane < k ? L.cb[lane] : INF;
    const uint32_t bi = lane < k ? reinterpret_cast<const uint32_t*>(L.cb)[64 + lane] : EMPTY_ID;
    bool slow = __ballot(lane < k && !(bd < INF)) != 0;
    int rk = 0;  // lane j < k: the candidates below candidate j
    int lb = 0;  // lane j < k: the list entries (of the first ef) below candidate j
    if (!slow) {
        int eq = 0;
        for (int j = 0; j < k; ++j) {
            const float dj = rl_f(bd, j);
            rk += dj < bd ? 1 : 0;
            eq += dj == bd ? 1 : 0;
        }
        slow = __ballot(lane < k && eq > 1) != 0;
    }
    if (!slow) {
        if (lane < k) {
            // (the steps add up to 2 LL_MAX_EF - 1 >= ef, so lb can reach ef)
#pragma unroll
            for (int step = LL_MAX_EF; step >= 1; step >>= 1) {
                const int t = lb + step - 1;
                if (t < ef && L.d[t] < bd) lb += step;
            }
        }
        slow = __ballot(lane < k && (lb >= ef || L.d[lb < ef ? lb : 0] == bd)) != 0;
    }
    if (slow) {
        for (int j = 0; j < k; ++j) bl_insert(L, ef, rl_f(bd, j), rl_u(bi, j));
        return;
    }
    // the distances are distinct: the best candidate has the lowest insertion
    // point (and the lowest new place), the worst the highest
    const int n = L.n;
    const int minlb = rl_i(lb, __ffsll((long long)__ballot(lane < k && rk == 0)) - 1);
    const int maxlb = rl_i(lb, __ffsll((long long)__ballot(lane < k && rk == k - 1)) - 1);
    for (int c = (n - 1) >> 6; c >= (minlb >> 6); --c) {
        const int idx = c * 64 + lane;
        const bool in = idx >= minlb && idx < n;
        const float ed = in ? L.d[idx] : 0.f;
        const uint32_t ei = in ? L.i[idx] : 0u;
        int sh = k;  // the candidates placed at or before entry idx
        if (c * 64 < maxlb) {
            sh = 0;
            for (int j = 0; j < k; ++j) sh += idx >= rl_i(lb, j) ? 1 : 0;
        }
        wave_sync();
        if (in && idx + sh < ef) {
            L.d[idx + sh] = ed;
            L.i[idx + sh] = ei;
        }
        wave_sync();
    }
    const int pos = rk + lb;
    if (lane < k && pos < ef) {
        L.d[pos] = bd;
        L.i[pos] = bi;
    }
    wave_sync();
    // the lowest unexpanded entry moved up with the candidates placed at or
    // before it, unless a candidate (unexpanded) landed below it
    const int up = __popcll(__ballot(lane < k && lb <= L.nx));
    L.nx = min(L.nx + up, minlb);
    L.n = min(n + k, ef);
}

__device__ __forceinline__ int bl_seed(const LList& L, uint32_t* vis, int vsize) {
    int seeded = 0;
    for (int b = 0; b < L.n; b += 64) {
        const int idx = b + lane_id();
        const bool ins = idx < L.n && vis_any_probe(vis, vsize, L.i[idx] & ID_MASK) == 1;
        seeded += __popcll(__ballot(ins));
    }
    return seeded;
}

// What the query kernels' one body (beam.hpp beam_query) asks of its list
// besides beam_layer_l's operations:
//   bl_regs<LT>            its registers per lane, R of BList<R>; 0: the list
//                          lives in LDS (LList)
//   bl_merges<LT>          its layer-0 steps go through bl_merge: lists of 256 /
//                          512 entries in registers, and every LDS list
//   bl_place(L, mem, efl)  the list's LDS part goes to mem (beam.hpp beam_lds
//                          says where that is and how long); returns beam_layer_l's mrg
//   bl_span(L)             the entries to scan for the outputs, in chunks of 64 from
//                          entry 0: 64 R, or the filled part of the LDS list
//   bl_chunk_id(L, e)      the chunk at entry e (a multiple of 64): entry e + lane's
//                          id word in each lane (EMPTY_ID past the filled entries),
//                          and bl_chunk_dist(L, e) its distance (read only for an
//                          entry that is there)
template <class LT>
constexpr int bl_regs = -1;  // (only these two lists: another type finds none of the bl_* overloads)
template <>
inline constexpr int bl_regs<LList> = 0;
template <int R>
constexpr int bl_regs<BList<R>> = R;
template <class LT>
constexpr bool bl_merges = bl_regs<LT> == 0 || bl_regs<LT> >= 4;

template <int R>
__device__ __forceinline__ float* bl_place(BList<R>&, uint32_t* mem, int) {
    return bl_merges<BList<R>> ? reinterpret_cast<float*>(mem) : nullptr;  // (bl_merge's scratch, BL_MERGE_WORDS)
}
__device__ __forceinline__ float* bl_place(LList& L, uint32_t* mem, int efl) {
    ll_place(L, mem, efl);
    return nullptr;  // (the candidate buffer is part of the list: bl_cbuf)
}

// (BList: e is the index of an unrolled loop, so the registers are indexed at compile time)
template <int R>
__device__ __forceinline__ constexpr int bl_span(const BList<R>&) {
    return R * 64;
}
template <int R>
__device__ __forceinline__ uint32_t bl_chunk_id(const BList<R>& L, int e) {
    return L.i[e >> 6];
}
template <int R>
__device__ __forceinline__ float bl_chunk_dist(const BList<R>& L, int e) {
    return L.d[e >> 6];
}
__device__ __forceinline__ int bl_span(const LList& L) { return L.n; }
__device__ __forceinline__ uint32_t bl_chunk_id(const LList& L, int e) {
    const int idx = e + lane_id();
    return idx < L.n ? L.i[idx] : EMPTY_ID;
}
__device__ __forceinline__ float bl_chunk_dist(const LList& L, int e) { return L.d[e + lane_id()]; }

// How beam_layer scores one batch of new candidates (ids in lanes 0..cnt-1 of
// cid) and hands the survivors to its sink: WaveBatch does it on the calling
// wave; the multi-wave single-query kernel (beam.hpp MwBatch) spreads the rows
// over the workgroup's waves.  Returns the rows evaluated in f32.
struct WaveBatch {
    template <class C, int G, bool SCREEN, class Sink>
    __device__ __forceinline__ int score(const GraphDev& g, const QReg<C>& q, float qn, uint32_t cid, int cnt,
                                         float wd, bool screen, float margin, Sink&& sink,
                                         unsigned long long& s16) const {
        if (SCREEN && screen && wd < __int_as_float(0x7f800000))
            return eval_screened<C, G>(g, q, qn, cid, cnt, g.metric, wd, sink, s16, margin);
        eval_list<C, G>(g, q, qn, cid, cnt, g.metric, sink);
        return cnt;
    }
};

// ---------------------------------------------------------------------------
// The layer-0 filter policy of beam_layer_l (DESIGN.md "Filtered search").
// NoFilter: the plain search, nothing added.  RowFilter: a second sorted list
// R (registers, capacity E <= 128) of the rows met that the query's allow-list
// holds and that are not deleted.  The route list L keeps routing through
// every row; a step offers a row to either list only when it beats both lists'
// worst entries as they stood BEFORE the step, L keeps its best W and R its
// best E of what was offered (so the arrival order inside a step is
// immaterial), and the search stops at the first unexpanded entry that R's
// worst entry precedes.  The result is R.
// ---------------------------------------------------------------------------
struct NoFilter {
    static constexpr bool on = false;
};
struct RowFilter {
    static constexpr bool on = true;
    const uint32_t* bits;  // row id -> bit, 32 rows a word (nullptr: every live row)
    int E;                 // R's capacity: max(ef, k) <= 128
    BList<2> R;
    // lane-parallel: is row id (< g.capn) in the allow-set
    __device__ __forceinline__ bool allowed(const GraphDev& g, uint32_t id) const {
        const bool bit = bits ? ((bits[id >> 5] >> (id & 31)) & 1u) != 0 : true;
        return bit && !is_dead(g, id);
    }
};

// ---------------------------------------------------------------------------
// beam: sorted list of <= ef entries; stop when every entry is expanded
// ---------------------------------------------------------------------------
// XW: entries expanded per step.  1 is the standard best-first search (the
// oracle's beam_layer_search with xw 1).  XW > 1 (the batched insert's layer
// searches, option "build_expand"; the query search's layer 0, option
// "search_expand"): the XW best unexpanded entries are expanded together --
// their adjacency rows fetched in one round trip and their new neighbours
// evaluated in batches of up to 64 against the worst entry before the step --
// fewer dependent round trips for a search whose expansions yield few new
// candidates.  The oracle restates it (beam_layer_search's xw).
// MH_SCREEN_PAD (a build flag for tools/ variants, default 0): widens the
// screen's margin, to measure how the rejections fall off with a looser bound
#ifndef MH_SCREEN_PAD
#define MH_SCREEN_PAD 0.f
#endif
// MERGE (the query search's layer 0 at ef > 128): the step's candidates go
// through bl_merge once per step, with `mrg` (BL_MERGE_WORDS of LDS) as its
// scratch.
// LT: the list, BList<R> (registers) or LList (LDS).
// Flt: the filter policy (NoFilter; RowFilter with the LDS list, XW 1 and MERGE,
// where a step is one batch, so "before the step" is "before the batch").
template <class C, class LT, int G, bool COH, bool SCREEN, int XW, bool MERGE, class BEv, class Flt>
__device__ __forceinline__ void beam_layer_l(const GraphDev& g, int layer, uint32_t entry, int ef, const QReg<C>& q,
                                             float qn, LT& L, uint32_t* vis, int vsize, WaveStats& st, const BEv& bev,
                                             float* mrg, Flt& flt) {
    static_assert(!Flt::on || (XW == 1 && MERGE && bl_regs<LT> == 0), "the filter runs on the LDS list, one entry a step");
    const int lane = lane_id();
    bl_init(L);
    if constexpr (Flt::on) bl_init(flt.R);
    if (entry == EMPTY_ID) return;
    vis_any_clear(vis, vsize);
    wave_sync();  // (the list and the visited set belong to this wave alone)
    if (lane == 0) vis_any_probe(vis, vsize, entry);
    int vcount = 1;
    if constexpr (Flt::on) {
        const bool ok = flt.allowed(g, guard_id(g, entry));  // (uniform)
        eval_list<C, G>(g, q, qn, entry, 1, g.metric, [&](float d, uint32_t u) {
            bl_insert(L, ef, d, u);
            if (ok) bl_insert(flt.R, flt.E, d, u);
        });
    } else {
        eval_list<C, G>(g, q, qn, entry, 1, g.metric, [&](float d, uint32_t u) { bl_insert(L, ef, d, u); });
    }
    st.E += 1;
    st.F += 1;
    const bool screen = SCREEN && h16_query_ok(qn);
    float margin = 0.f;  // the copy's measured rounding -> the metric's screening margin
    if constexpr (SCREEN) {
        const float e = g.h16err ? *g.h16err : 0.00048828125f;
        margin = g.metric == EUCLIDEAN ? h16_margin_l2(e) : h16_margin_cos(e);
        margin += MH_SCREEN_PAD;
    }
    const int32_t* degp = g.layers[layer].deg;
    const int32_t* adjp = g.layers[layer].adj;
    const int capl = g.layers[layer].cap;
#ifdef MH_PROF_BEAM
    const unsigned long long tl0 = clock64();
    struct AllClock {  // adds the layer-0 search's cycles at every exit
        WaveStats& st;
        unsigned long long t0;
        int layer;
        __device__ ~AllClock() {
            if (layer == 0) st.c_all += clock64() - t0;
        }
    } all_clock{st, tl0, layer};
#endif
    for (;;) {
        uint32_t cur[XW];
        cur[0] = bl_next(L);
        if (cur[0] == EMPTY_ID) break;
        float rwd = __int_as_float(0x7f800000);  // Flt: R's worst entry before the step
        uint32_t rwi = EMPTY_ID;
        if constexpr (Flt::on) {
            bl_at(flt.R, flt.E - 1, rwd, rwi);
            // R is full and its worst entry precedes the best unexpanded one:
            // nothing left can improve the results
            if (rwi != EMPTY_ID && lt_di(rwd, rwi, bl_picked_dist(L), cur[0] & ID_MASK)) break;
        }
#pragma unroll
        for (int w = 1; w < XW; ++w) cur[w] = bl_next(L);
        // the adjacency rows are loaded together with their degrees (rows are
        // cap wide, so lanes past the degree read allocated, ignored slots):
        // one dependent round trip per step
        int32_t rowv[XW];
        int deg[XW];
#pragma unroll
        for (int w = 0; w < XW; ++w) {
            rowv[w] = -1;
            deg[w] = 0;
            if (cur[w] != EMPTY_ID) {
                st.X += 1;
                const uint32_t cg = guard_id(g, cur[w]);
                rowv[w] = lane < capl ? ld_i32<COH>(adjp + (size_t)cg * capl + lane) : -1;
                deg[w] = min(uni(ld_i32<COH>(degp + cg)), capl);
            }
        }
        uint32_t cids[XW];
        int cnts[XW];
        bool cok = false;  // Flt: lane t < cnts[0]: candidate t is in the allow-set
#pragma unroll
        for (int w = 0; w < XW; ++w) {
            const bool have = lane < deg[w];
            uint32_t nb = have ? (uint32_t)rowv[w] : 0u;
            int pr = 0;
            bool ok = false;
            if (have && nb != 0xFFFFFFFFu) {
                nb = guard_id(g, nb);
                if constexpr (Flt::on) ok = flt.allowed(g, nb);  // one gather a step, beside the probe
                pr = vis_any_probe(vis, vsize, nb);
            }
            vcount += __popcll(__ballot(pr == 1));
            cids[w] = compact(nb, pr != 0, cnts[w]);
            if constexpr (Flt::on) {
                int c2;
                cok = compact(ok ? 1u : 0u, pr != 0, c2) != 0 && lane < c2;
            }
        }
        // the new neighbours of consecutive expanded entries share a batch while
        // they fit the wave
        if constexpr (XW >= 2) {
            int b = 0;
#pragma unroll
            for (int w = 1; w < XW; ++w) {
                if (cnts[b] + cnts[w] <= 64) {
                    const uint32_t cw = shfl_u(cids[w], (lane - cnts[b]) & 63);
#pragma unroll
                    for (int v = 0; v < w; ++v)  // (static register indices)
                        if (v == b && lane >= cnts[v]) cids[v] = cw;
#pragma unroll
                    for (int v = 0; v < w; ++v)
                        if (v == b) cnts[v] += cnts[w];
                    cnts[w] = 0;
                } else {
                    b = w;
                }
            }
        }
        float wd = __int_as_float(0x7f800000);
        uint32_t wi = EMPTY_ID;
        if constexpr (SCREEN || MERGE) bl_at(L, ef - 1, wd, wi);  // the worst before the step: it only decreases during it
        // Flt: the screen's threshold is the lower of the two lists' worst distances
        // (what the copy proves worse than it is offered to neither list)
        const float sd = Flt::on ? fminf(wd, rwd) : wd;
        int bk = 0;  // MERGE: the step's candidates below that worst, in mrg's buffer
        // the batches are taken from slot 0 and the slots shifted down, so every
        // register index is static whether or not the compiler unrolls this loop
        // (a large score() body can keep it rolled)
        for (int w = 0; w < XW; ++w) {
            const int cnt = cnts[0];
            const uint32_t cid = cids[0];
#pragma unroll
            for (int v = 0; v + 1 < XW; ++v) {
                cnts[v] = cnts[v + 1];
                cids[v] = cids[v + 1];
            }
            cnts[XW - 1] = 0;
            if (cnt == 0) continue;
            st.E += cnt;
            if constexpr (MERGE) {
                {
                    if (bk + cnt > 64) {  // (a batch adds at most cnt)
                        bl_merge(L, ef, bk, mrg);
                        bk = 0;
                    }
                    float* cb = bl_cbuf(L, mrg);
                    if constexpr (Flt::on) {
                        // offered: below both worst entries as saved before the step (R's
                        // live bound falls inside the step; the saved one decides)
                        auto sink = [&](float d, uint32_t u) {
                            if (lt_di(d, u, wd, wi & ID_MASK) && lt_di(d, u, rwd, rwi)) {
                                if (lane == 0) {
                                    cb[bk] = d;
                                    reinterpret_cast<uint32_t*>(cb)[64 + bk] = u;
                                }
                                ++bk;
                                if (__ballot(lane < cnt && cid == u && cok) != 0) bl_insert(flt.R, flt.E, d, u);
                            }
                        };
                        st.F += bev.template score<C, G, SCREEN>(g, q, qn, cid, cnt, sd, screen, margin, sink, st.S);
                        continue;
                    }
                    auto sink = [&](float d, uint32_t u) {
                        if (lt_di(d, u, wd, wi & ID_MASK)) {
                            if (lane == 0) {
                                cb[bk] = d;
                                reinterpret_cast<uint32_t*>(cb)[64 + bk] = u;
                            }
                            ++bk;
                        }
                    };
                    st.F += bev.template score<C, G, SCREEN>(g, q, qn, cid, cnt, wd, screen, margin, sink, st.S);
                    continue;
                }
            }
#ifdef MH_PROF_BEAM
            const unsigned long long t0 = clock64();
            unsigned long long ti = 0;
            auto sink = [&](float d, uint32_t u) {
                const unsigned long long a = clock64();
                bl_insert(L, ef, d, u);
                ti += clock64() - a;
            };
            st.F += bev.template score<C, G, SCREEN>(g, q, qn, cid, cnt, wd, screen, margin, sink, st.S);
            if (layer == 0) {
                st.c_ins += ti;
                st.c_score += clock64() - t0 - ti;
            }
#else
            auto sink = [&](float d, uint32_t u) { bl_insert(L, ef, d, u); };
            st.F += bev.template score<C, G, SCREEN>(g, q, qn, cid, cnt, wd, screen, margin, sink, st.S);
#endif
        }
        if constexpr (MERGE) {
            if (bk > 0) bl_merge(L, ef, bk, mrg);
        }
        if (vcount > MH_VIS_FULL(vis_any_cap(vsize))) {  // reset: results unchanged
            wave_sync();
            vis_any_clear(vis, vsize);
            wave_sync();
            vcount = bl_seed(L, vis, vsize);  // the list's members stay visited
            wave_sync();
            st.resets += 1;
        }
    }
}

template <class C, int R, int G, bool COH = false, bool SCREEN = false, int XW = 1, bool MERGE = false,
          class BEv = WaveBatch>
__device__ __forceinline__ void beam_layer(const GraphDev& g, int layer, uint32_t entry, int ef, const QReg<C>& q, float qn,
                           BList<R>& L, uint32_t* vis, int vsize, WaveStats& st, const BEv& bev = BEv(),
                           float* mrg = nullptr) {
    NoFilter nf;
    beam_layer_l<C, BList<R>, G, COH, SCREEN, XW, MERGE, BEv>(g, layer, entry, ef, q, qn, L, vis, vsize, st, bev, mrg, nf);
}

// ---------------------------------------------------------------------------
// several waves per query (or insert): wave 0 runs the list, the visited set
// and the expansions; each batch of new candidates is split over the waves
// (screen + f32 on each wave's rows, in one round trip instead of one per 16
// rows) and the survivors come back to wave 0's list.  The list is the best ef
// of everything inserted whatever the insertion order, so the results are the
// one-wave kernel's bit for bit (k_search_beam_mw, k_batch_search_mw).
// ---------------------------------------------------------------------------
constexpr int BMW_WAVES = 4;
constexpr int BMW_SCORE = 0, BMW_EXIT = 1;
struct BmwShare {
    int cmd, cnt;
    float wd;
    int pad_;
    uint32_t list[64];
    int scnt[BMW_WAVES];
    float sd[BMW_WAVES * 64];
    uint32_t si[BMW_WAVES * 64];
};

// everything handed between the waves is in LDS (rows and norms are only read)
__device__ __forceinline__ void bmw_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// wave w's rows of the posted batch, [w*ch, min(cnt, (w+1)*ch)): screened
// against the posted worst, survivors (f32 distance, id) into sd / si
template <class C, int G, bool SCREEN>
__device__ __forceinline__ int bmw_share(const GraphDev& g, const QReg<C>& q, float qn, BmwShare* sh, int w,
                                         bool screen, float margin, unsigned long long& s16) {
    const int lane = lane_id();
    const int cnt = uni(sh->cnt);
    const float wd = __int_as_float(uni(__float_as_int(sh->wd)));
    const int ch = (cnt + BMW_WAVES - 1) / BMW_WAVES;
    const int t0 = w * ch;
    const int c = min(cnt - t0, ch);
    int k = 0, f = 0;
    if (c > 0) {
        const uint32_t cid = lane < c ? sh->list[t0 + lane] : 0u;
        auto sink = [&](float d, uint32_t u) {
            if (lane == 0) {
                sh->sd[w * 64 + k] = d;
                sh->si[w * 64 + k] = u;
            }
            ++k;
        };
        f = WaveBatch().template score<C, G, SCREEN>(g, q, qn, cid, c, wd, screen, margin, sink, s16);
    }
    if (lane == 0) sh->scnt[w] = k;
    return f;
}

struct MwBatch {
    BmwShare* sh;
    template <class C, int G, bool SCREEN, class Sink>
    __device__ __forceinline__ int score(const GraphDev& g, const QReg<C>& q, float qn, uint32_t cid, int cnt,
                                         float wd, bool screen, float margin, Sink&& sink,
                                         unsigned long long& s16) const {
        const int lane = lane_id();
        if (lane < cnt) sh->list[lane] = cid;
        if (lane == 0) {
            sh->cmd = BMW_SCORE;
            sh->cnt = cnt;
            sh->wd = wd;
        }
        bmw_barrier();  // post
        const int f = bmw_share<C, G, SCREEN>(g, q, qn, sh, 0, screen, margin, s16);
        bmw_barrier();  // collect
#pragma unroll
        for (int w = 0; w < BMW_WAVES; ++w) {
            const int n = uni(sh->scnt[w]);
            const float dv = lane < n ? sh->sd[w * 64 + lane] : 0.f;
            const uint32_t iv = lane < n ? sh->si[w * 64 + lane] : 0u;
            for (int t = 0; t < n; ++t) sink(rl_f(dv, t), rl_u(iv, t));
        }
        return f;  // this wave's rows (the others count theirs)
    }
};


// ---------------------------------------------------------------------------
// compat: graph.go:94-170 verbatim semantics on LDS Go-heaps
// ---------------------------------------------------------------------------
struct CompatSmem {
    uint32_t* vis;
    int vlog2;
    float* cd;
    uint32_t* ci;  // candidates heap [ef+2]
    float* rd;
    uint32_t* ri;  // result heap [k+2]
};

// HP: GHeap (LDS arrays S.cd/S.ci and S.rd/S.ri) or RHeap (one slot per lane,
// when ef + 1 and k + 1 fit the wave); the result heap ends in S.rd / S.ri
// either way, in heap order.
template <class C, int G, bool COH, class Ev, class HP>
__device__ __forceinline__ int compat_layer_h(const GraphDev& g, int layer, uint32_t entry, int k, int ef,
                                              const QReg<C>& q, float qn, CompatSmem& S, WaveStats& st, int& err,
                                              const Ev& ev, HP cand, HP res) {
    const int lane = lane_id();
    const int vsize = 1 << S.vlog2, vmask = vsize - 1;
    vis_clear(S.vis, vsize);
    ev.sync();
    float d0 = 0.f;
    ev.template run<C, G>(g, q, qn, entry, 1, g.metric, [&](float d, uint32_t) { d0 = d; });  // graph.go:112
    st.E += 1;
    if (lane == 0) vis_probe(S.vis, vmask, kid_of(g, entry));  // graph.go:123 visited[n.Key]
    hp_push(cand, d0, entry);                          // graph.go:109-114
    hp_push(res, hp_d(cand, 0), hp_id(cand, 0));       // graph.go:122
    const int32_t* degp = g.layers[layer].deg;
    const int32_t* adjp = g.layers[layer].adj;
    const int capl = g.layers[layer].cap;
    while (cand.n > 0) {
        float cdist;
        uint32_t cur;
        hp_pop(cand, cdist, cur);  // graph.go:127
        bool improved = false;
        const uint32_t cg = guard_id(g, cur);
        // the row is loaded with its degree (one round trip, entries past deg ignored)
        const int32_t rowv = lane < capl ? ld_i32<COH>(adjp + (size_t)cg * capl + lane) : -1;
        const int deg = min(uni(ld_i32<COH>(degp + cg)), capl);
        if (deg < 0) continue;  // graph.go:131-133 (nil neighbor map)
        st.X += 1;
        const bool have = lane < deg;
        uint32_t nb = 0xFFFFFFFFu;
        int64_t key = INT64_MAX;
        if (have) {
            nb = guard_id(g, (uint32_t)rowv);
            key = g.keys[nb];
        }
        rank_sort(key, nb, deg);  // graph.go:137-138 ascending key order
        int pr = 0;
        if (lane < deg) pr = vis_probe(S.vis, vmask, kid_of(g, nb));  // graph.go:141-144 (by key)
        if (__ballot(pr == 2)) err = 1;                   // exact visited set required here
        int cnt;
        const uint32_t cid = compact(nb, pr == 1, cnt);
        st.E += cnt;
        CPROF_T(tq);
        ev.template run<C, G>(g, q, qn, cid, cnt, g.metric, [&](float dist, uint32_t u) {  // graph.go:146-159
            improved = improved || (res.n > 0 && dist < hp_d(res, 0));
            if (res.n < k) {
                hp_push(res, dist, u);
            } else if (dist < hp_d(res, res.n - 1)) {
                hp_poplast(res);
                hp_push(res, dist, u);
            }
            hp_push(cand, dist, u);
            if (cand.n > ef) hp_poplast(cand);
        });
        CPROF_ADD(tq, 22);
        CPROF_CNT(23, cnt);
        if (!improved && res.n >= k) break;  // graph.go:164-166
    }
    hp_store(res, S.rd, S.ri);
    return res.n;
}

template <class C, int G, bool COH = false, class Ev = WaveEval>
__device__ __forceinline__ int compat_layer(const GraphDev& g, int layer, uint32_t entry, int k, int ef, const QReg<C>& q, float qn,
                            CompatSmem& S, WaveStats& st, int& err, const Ev& ev = Ev()) {
    if (entry == EMPTY_ID) return 0;
    if (ef < 64 && k < 64)  // at most ef + 1 / k + 1 entries at a time
        return compat_layer_h<C, G, COH>(g, layer, entry, k, ef, q, qn, S, st, err, ev, RHeap{}, RHeap{});
    return compat_layer_h<C, G, COH>(g, layer, entry, k, ef, q, qn, S, st, err, ev, GHeap{S.cd, S.ci, 0},
                                     GHeap{S.rd, S.ri, 0});
}

}  // namespace mh
