// build_compat.hpp -- the reference's strictly sequential insert and delete
// (Graph.Add / BatchAdd, graph.go:437-531, 942-1042; Delete / BatchDelete,
// graph.go:843-895), verbatim semantics, instantiated per configuration in
// build_units.hip.  One wave walks the inserts in order.  Graph state is rewritten
// while it is searched, so adjacency goes through relaxed atomics + __syncthreads.
#pragma once
#include <algorithm>

#include "device_search.hpp"
#include "engine.hpp"

namespace mh {

// waves: 1 (k_build_compat) or 8 (k_build_compat_mw)
template <int L, int V>
int launch_build_compat_cfg(const CompatBuildArgs& a, int waves, hipStream_t s);
template <int L, int V>
int launch_delete_compat_cfg(const DeleteArgs& a, hipStream_t s);

// ---------------------------------------------------------------------------
// compat build
// ---------------------------------------------------------------------------
// The walks below run on ONE wave (the "master"): every graph mutation, heap
// and visited-set operation happens there, in the reference's order.  Only
// distance batches are delegated, through the evaluator policy `Ev`:
// WaveEval evaluates on the master itself; MwEval (k_build_compat_mw) hands a
// batch to all waves of the workgroup and gets the distances back in LDS, in
// the same order.  Distances are the canonical ones whichever wave computes
// them (eval_rows), so both evaluators give identical graphs.
struct BuildSmem {
    CompatSmem cs;
    float* hd;  // replenish heap
    uint32_t* hi;
    int hcap;
    uint32_t* radj;  // replenish: staged neighbour rows (hcap entries)
    int64_t* rkey;   // ... and their keys
    // eviction speculation (k_build_compat_mw): the neighbourhood's rows as the
    // layer's addNeighbor pairs start, each followed by the new node, and the
    // distances of every such entry to its row's owner (stride pstride)
    int32_t* prow = nullptr;  // [pgroups * pstride] entry i of neighbour j's row
    int* pdeg = nullptr;      // [pgroups] its degree (-1 nil)
    float* pdist = nullptr;   // [pgroups * pstride] distance of entry i to neighbour j (entry deg: the new node)
    int pgroups = 0, pstride = 0;
};

// Rows are loaded together with their degree (one round trip; entries past
// the degree are ignored): the sequential walk is bound by dependent loads.
// list_remove_in: n's row already in registers (lane i: entry i, d entries);
// both are updated to the row after the removal, so the next step on n (the
// replenish after an eviction) needs no reload.
template <class Ev>
__device__ __forceinline__ void list_remove_in(const GraphDev& g, int l, uint32_t n, int32_t& rv, int& d, uint32_t v,
                                               const Ev& ev) {
    const int lane = lane_id();
    if (d <= 0) return;
    // delete(n.neighbors, v.Key): the entry of v's key, whichever row it holds
    const bool hit = lane < d && kid_of(g, guard_id(g, (uint32_t)rv)) == kid_of(g, v);
    const unsigned long long m = __ballot(hit);
    if (!m) return;
    const int pos = __ffsll((long long)m) - 1;
    const int32_t last = __shfl(rv, d - 1, 64);
    ev.sync();
    if (lane == 0) {
        st_i32(g.layers[l].adj + (size_t)n * g.layers[l].cap + pos, last);
        st_i32(g.layers[l].deg + n, d - 1);
    }
    ev.sync();
    if (lane == pos) rv = last;
    d = d - 1;
}
template <class C, int G, class Ev>
__device__ __forceinline__ void list_remove(const GraphDev& g, int l, uint32_t n, uint32_t v, const Ev& ev) {
    const int lane = lane_id();
    const int capl = g.layers[l].cap;
    int32_t rv = lane < capl ? ld_i32<true>(g.layers[l].adj + (size_t)n * capl + lane) : -1;
    int d = uni(ld_i32<true>(g.layers[l].deg + n));  // uniform: scalar loop bounds
    list_remove_in(g, l, n, rv, d, v, ev);
}

// graph.go:50 n.neighbors[nw.Key] = nw: overwrite the entry of nw's key (which
// may hold another row of that key), else append; returns the new degree and,
// in *rowout (nullable), the row after the assignment (lane i: entry i)
template <class Ev>
__device__ __forceinline__ int list_append(const GraphDev& g, int l, uint32_t n, uint32_t nw, const Ev& ev,
                           int32_t* rowout = nullptr) {
    const int lane = lane_id();
    const int capl = g.layers[l].cap;
    int32_t* row = g.layers[l].adj + (size_t)n * capl;
    const int32_t rv = lane < capl ? ld_i32<true>(row + lane) : -1;
    int d = uni(ld_i32<true>(g.layers[l].deg + n));
    if (d < 0) d = 0;  // graph.go:46-48 allocate the map
    const bool pres = lane < d && kid_of(g, guard_id(g, (uint32_t)rv)) == kid_of(g, nw);
    const unsigned long long pm = __ballot(pres);
    const bool present = pm != 0;
    const int pos = present ? __ffsll((long long)pm) - 1 : d;
    const int nd = uni(present ? d : d + 1);  // (computed outside the lane-0 stores: stays scalar)
    ev.sync();
    if (lane == 0) {
        st_i32(row + pos, (int32_t)nw);
        st_i32(g.layers[l].deg + n, nd);
    }
    ev.sync();
    if (rowout) *rowout = lane == pos ? (int32_t)nw : rv;
    return nd;
}

// graph.go:172-219 when the outcome does not depend on the walk order.  With
// one row per key (no replaced keys: g.kid == nullptr) the candidates are a SET
// -- neighbours of neighbours, minus n and its neighbours, one per key -- and
// when the pops it takes are strict minima (no NaN, no tie at any pop) every
// heap shape pops the same rows in the same order.  So: stage the rows without
// their keys, collect the set through the visited table in any lane order,
// score it, and check the pops before making any of them.  Returns false
// (nothing changed) when a NaN or a tie needs the reference's exact push
// order; replenish then takes the ordered walk.
template <class C, int G, class Ev>
__device__ __forceinline__ bool replenish_set(const GraphDev& g, int l, uint32_t n, int m, int dn, int32_t rv, BuildSmem& S,
                              WaveStats& st, int& err, const Ev& ev) {
    const int lane = lane_id();
    const int capl = g.layers[l].cap;
    const uint32_t mine = lane < dn ? guard_id(g, (uint32_t)rv) : 0u;
    const int mydeg = lane < dn ? min(ld_i32<true>(g.layers[l].deg + mine), capl) : -1;
    const int tot = min(dn * capl, S.hcap);
    const int vsize = 1 << S.cs.vlog2, vmask = vsize - 1;
    vis_clear(S.cs.vis, vsize);
    ev.sync();
    if (lane == 0) vis_probe(S.cs.vis, vmask, n);     // graph.go:184
    if (lane < dn) vis_probe(S.cs.vis, vmask, mine);  // graph.go:187-189
    ev.sync();
    int ncand = 0;
    constexpr int U = 4;  // rows' entries in flight per pass
    for (int e0 = 0; e0 < tot; e0 += 64 * U) {
        int32_t x[U];
        int dj[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {  // uniform trip count: the shuffles see every lane
            const int e = e0 + u * 64 + lane;
            const int j = min(e / capl, 63), i = e % capl;
            const uint32_t nb = shfl_u(mine, j);
            x[u] = e < tot && j < dn ? ld_i32<true>(g.layers[l].adj + (size_t)nb * capl + i) : -1;
            dj[u] = __shfl(mydeg, j, 64);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int e = e0 + u * 64 + lane;
            const int i = e % capl;
            uint32_t v = EMPTY_ID;
            if (e < tot && i < dj[u]) v = guard_id(g, (uint32_t)x[u]);
            int pr = 0;
            if (v != EMPTY_ID) pr = vis_probe(S.cs.vis, vmask, v);  // graph.go:198-201
            if (__ballot(pr == 2)) err = 1;
            int cnt;
            const uint32_t cid = compact(v, pr == 1, cnt);
            if (ncand + cnt > S.hcap) {
                err |= 8;
                cnt = S.hcap - ncand;
            }
            if (lane < cnt) ev.list[ncand + lane] = cid;
            ncand += cnt;
        }
    }
    ev.sync();
    st.E += ncand;
    CPROF_CNT(19, ncand);
    {
        QReg<C> q;
        load_query(q, g.vecs + (size_t)n * g.pitch);
        ev.template score<C, G>(g, q, g.norms[n], ncand, COSINE, S.hd, S.hi);  // graph.go:204 hard-coded cosine
    }
    ev.sync();
    bool anynan = false;
    for (int e = lane; e < ncand; e += 64) anynan |= !(S.hd[e] == S.hd[e]);
    const int need = min(m - dn, ncand);  // each pop adds a new key: deg grows by one
    if (__ballot(anynan) || need > 64) return false;
    uint32_t popped = 0xFFFFFFFFu;  // lane p: the candidate index of pop p
    for (int p = 0; p < need; ++p) {
        float mv = __int_as_float(0x7f800000);
        int mi = -1;
        for (int e = lane; e < ncand; e += 64) {
            bool gone = false;
            for (int j = 0; j < p; ++j) gone |= rl_u(popped, j) == (uint32_t)e;
            const float v = S.hd[e];
            if (!gone && (mi < 0 || v < mv)) {
                mv = v;
                mi = e;
            }
        }
        float wm = mi < 0 ? __int_as_float(0x7f800000) : mv;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) wm = fminf(wm, __shfl_xor(wm, o, 64));
        int eq = 0;
        for (int e = lane; e < ncand; e += 64) {
            bool gone = false;
            for (int j = 0; j < p; ++j) gone |= rl_u(popped, j) == (uint32_t)e;
            eq += (!gone && S.hd[e] == wm) ? 1 : 0;
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) eq += __shfl_xor(eq, o, 64);
        if (eq != 1) return false;  // a tie: the heap's shape decides
        const unsigned long long own = __ballot(mi >= 0 && mv == wm);
        const int bi = __shfl(mi, __ffsll((long long)own) - 1, 64);
        if (lane == p) popped = (uint32_t)bi;
    }
    CPROF_CNT(15, 1);
    for (int p = 0; p < need; ++p) list_append(g, l, n, S.hi[rl_u(popped, p)], ev);  // graph.go:213-218
    return true;
}

// graph.go:172-219.  The neighbours' rows and keys are staged in LDS in one
// pass (instead of one dependent load chain per neighbour); the candidates are
// then collected in the reference's walk order (neighbours, then their
// neighbours, both in ascending key order -- the map-order stand-in) for all
// rows at once, and ONE distance batch scores them all; the heap sees the
// pushes in the same order as a per-neighbour loop would produce.
template <class C, int G, class Ev>
__device__ __forceinline__ void replenish(const GraphDev& g, int l, uint32_t n, int m, BuildSmem& S, WaveStats& st, int& err,
                          const Ev& ev, const int32_t* known_row = nullptr, int known_deg = 0) {
    const int lane = lane_id();
    const int capl = g.layers[l].cap;
    // n's row and degree: from the caller's registers when it just changed them
    const int32_t rv = known_row ? *known_row : lane < capl ? ld_i32<true>(g.layers[l].adj + (size_t)n * capl + lane) : -1;
    int dn = known_row ? known_deg : uni(ld_i32<true>(g.layers[l].deg + n));
    if (dn < 0) dn = 0;
    if (dn >= m) return;
    CPROF_T(tr);
    CPROF_CNT(18, 1);
    if (!g.kid) {
        const bool done = replenish_set<C, G>(g, l, n, m, dn, rv, S, st, err, ev);
        CPROF_ADD(tr, 14);
        if (done) return;
        CPROF_CNT(20, 1);
    }
    uint32_t mine = 0xFFFFFFFFu;
    int64_t key = INT64_MAX;
    if (lane < dn) {
        mine = guard_id(g, (uint32_t)rv);
        key = g.keys[mine];
    }
    rank_sort(key, mine, dn);
    // stage every neighbour's row (deg, entries, keys) -- rows j < dn, j-major
    const int mydeg = lane < dn ? min(ld_i32<true>(g.layers[l].deg + mine), capl) : -1;
    const int tot = min(dn * capl, S.hcap);
    for (int e0 = 0; e0 < tot; e0 += 64) {  // uniform trip count: the shuffles see every lane
        const int e = e0 + lane;
        const int j = min(e / capl, 63), i = e % capl;
        const uint32_t nb = shfl_u(mine, j);
        // the entry load goes out before the degree is needed (masked below)
        const int32_t ev_ = e < tot && j < dn ? ld_i32<true>(g.layers[l].adj + (size_t)nb * capl + i) : -1;
        const int dj = __shfl(mydeg, j, 64);
        uint32_t th = 0xFFFFFFFFu;
        int64_t tk = INT64_MAX;
        if (e < tot && i < dj) {
            th = guard_id(g, (uint32_t)ev_);
            tk = g.keys[th];
        }
        if (e < tot) {
            S.radj[e] = th;
            S.rkey[e] = tk;
        }
    }
    ev.sync();
    CPROF_ADD(tr, 5);
    // The reference's walk (graph.go:184-210): visited = {n} + n's neighbours;
    // then each neighbour j in key order, each of its neighbours in key order,
    // collecting the ones not yet visited.  All rows at once: (1) every entry's
    // rank in its row's key order gives its walk position j*capl + rank in
    // S.hi (EMPTY past the row's degree); (2) a walk entry is collected when it
    // is not n, not one of n's neighbours and not seen at an earlier position.
    uint32_t* W = S.hi;
    for (int e0 = 0; e0 < tot; e0 += 64) {  // uniform trip count for the shuffle
        const int e = e0 + lane;
        const int j = min(e / capl, 63), i = e % capl;
        const int dj = __shfl(mydeg, j, 64);
        if (e < tot) {
            const uint32_t v = S.radj[e];
            const int64_t kv = S.rkey[e];
            const int row = j * capl;
            if (i < dj) {
                int r = 0;
#pragma unroll 8
                for (int i2 = 0; i2 < dj && row + i2 < tot; ++i2) {
                    const int64_t k2 = S.rkey[row + i2];
                    const uint32_t v2 = S.radj[row + i2];
                    r += (k2 < kv || (k2 == kv && (v2 < v || (v2 == v && i2 < i)))) ? 1 : 0;
                }
                W[row + r] = v;
            } else {
                W[e] = EMPTY_ID;
            }
        }
    }
    ev.sync();
    CPROF_ADD(tr, 6);
    const int vsize = 1 << S.cs.vlog2, vmask = vsize - 1;
    vis_clear(S.cs.vis, vsize);
    ev.sync();
    if (lane == 0) vis_probe(S.cs.vis, vmask, kid_of(g, n));     // graph.go:184 visited[n.Key]
    if (lane < dn) vis_probe(S.cs.vis, vmask, kid_of(g, mine));  // graph.go:187-189
    ev.sync();
    int ncand = 0;
    for (int e0 = 0; e0 < tot; e0 += 64) {  // 64 walk positions at a time, in order
        const int e = e0 + lane;
        const uint32_t v = e < tot ? W[e] : EMPTY_ID;
        const uint32_t kv = v != EMPTY_ID ? kid_of(g, v) : EMPTY_ID;  // graph.go:198 visited[k]: by key
        bool first = v != EMPTY_ID;  // not repeated at a lower lane of this chunk
#pragma unroll 9
        for (int l2 = 0; l2 < 63; ++l2) first = first && !(l2 < lane && rl_u(kv, l2) == kv);
        int pr = 0;
        if (first) pr = vis_probe(S.cs.vis, vmask, kv);  // earlier chunks and the pre-visited set
        if (__ballot(pr == 2)) err = 1;
        int cnt;
        const uint32_t cid = compact(v, pr == 1, cnt);
        if (ncand + cnt > S.hcap) {
            err |= 8;
            cnt = S.hcap - ncand;
        }
        if (lane < cnt) ev.list[ncand + lane] = cid;
        ncand += cnt;
    }
    ev.sync();
    CPROF_ADD(tr, 7);
    CPROF_CNT(19, ncand);
    st.E += ncand;
    // distances in push order (the reference pushes each into its heap)
    {
        QReg<C> q;
        load_query(q, g.vecs + (size_t)n * g.pitch);
        const float qn = g.norms[n];
        ev.template score<C, G>(g, q, qn, ncand, COSINE, S.hd, S.hi);  // graph.go:204 hard-coded cosine
    }
    ev.sync();
    CPROF_ADD(tr, 8);
    // graph.go:213-218 (len < m before every add: addNeighbor cannot evict).
    // Every Pop returns the heap's minimum.  While no distance is NaN and the
    // minimum of what is left is unique, that is the arg-min whatever shape
    // the heap has, so the pushes are skipped.  Otherwise the heap is built in
    // place by replaying the pushes (element e of the push-order array is the
    // e-th push), the pops made so far are replayed, and the walk continues on
    // the heap exactly as the reference's.
    bool anynan = false;
    for (int e = lane; e < ncand; e += 64) anynan |= !(S.hd[e] == S.hd[e]);
    bool fast = __ballot(anynan) == 0ull;
    uint32_t popped = 0xFFFFFFFFu;  // fast path: lane j holds the index of the j-th pop
    int npop = 0;
    GHeap h{S.hd, S.hi, 0};
    auto gone = [&](int e) {
        bool r = false;
        for (int j = 0; j < npop; ++j) r |= rl_u(popped, j) == (uint32_t)e;
        return r;
    };
    auto replay = [&]() {
        for (int e = 0; e < ncand; ++e) {
            h.n = e + 1;
            gh_up(h, e);
        }
        for (int j = 0; j < npop; ++j) {
            float bd;
            uint32_t bb;
            gh_pop(h, bd, bb);
        }
        fast = false;
    };
    if (!fast) replay();
    for (;;) {
        int cur = uni(ld_i32<true>(g.layers[l].deg + n));
        if (cur < 0) cur = 0;
        if (cur >= m) break;
        uint32_t best;
        if (fast) {
            if (npop >= ncand) break;
            float mv = __int_as_float(0x7f800000);
            int mi = -1;
            for (int e = lane; e < ncand; e += 64) {
                const float v = S.hd[e];
                if (!gone(e) && (mi < 0 || v < mv)) {
                    mv = v;
                    mi = e;
                }
            }
            float wm = mi < 0 ? __int_as_float(0x7f800000) : mv;
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) wm = fminf(wm, __shfl_xor(wm, o, 64));
            int eq = 0;
            for (int e = lane; e < ncand; e += 64) eq += (!gone(e) && S.hd[e] == wm) ? 1 : 0;
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) eq += __shfl_xor(eq, o, 64);
            if (eq == 1 && npop < 64) {
                const unsigned long long own = __ballot(mi >= 0 && mv == wm);
                const int bi = __shfl(mi, __ffsll((long long)own) - 1, 64);
                best = S.hi[bi];
                if (lane == npop) popped = (uint32_t)bi;
                ++npop;
            } else {
                replay();  // a tie at the minimum: the heap's shape decides
            }
        }
        if (!fast) {
            if (h.n <= 0) break;
            float bd;
            gh_pop(h, bd, best);
        }
        list_append(g, l, n, best, ev);
    }
    CPROF_ADD(tr, 9);
}

// What add_neighbor(n, nw) needs from before its own append, staged for the
// whole neighbourhood at once (compat_insert): n's row and degree, and the
// distance from n to each entry (entry deg: to nw).
struct EvictSpec {
    const int32_t* row;
    int deg;
    const float* dist;
};

// graph.go:41-81.  Returns the evicted neighbour (EMPTY_ID: none).
template <class C, int G, class Ev>
__device__ __forceinline__ uint32_t add_neighbor(const GraphDev& g, int l, uint32_t n, uint32_t nw, int m, BuildSmem& S,
                                                 WaveStats& st, int& err, const Ev& ev,
                                                 bool have_sp = false, EvictSpec sp = {}) {
    const int lane = lane_id();
    const int capl = g.layers[l].cap;
    int32_t rv;
    int d;
    float worst_d = -__int_as_float(0x7f800000);
    uint32_t worst = EMPTY_ID;
    bool decided = false;
    CPROF_T(ta);
    QReg<C> q;
    float qn = 0.f;
    if (have_sp) {
        // the append of list_append from the staged row (graph.go:50), then the
        // staged distances: entry i of the row after it is the old entry i, or
        // nw where nw went (the slot of its key, else slot deg)
        const int d0 = sp.deg < 0 ? 0 : sp.deg;  // graph.go:46-48 allocate the map
        const int32_t r0 = lane < capl ? sp.row[lane] : -1;
        const bool pres = lane < d0 && kid_of(g, guard_id(g, (uint32_t)r0)) == kid_of(g, nw);
        const unsigned long long pm = __ballot(pres);
        const int pos = pm ? __ffsll((long long)pm) - 1 : d0;
        d = uni(pm ? d0 : d0 + 1);
        ev.sync();
        if (lane == 0) {
            st_i32(g.layers[l].adj + (size_t)n * capl + pos, (int32_t)nw);
            st_i32(g.layers[l].deg + n, d);
        }
        ev.sync();
        rv = lane == pos ? (int32_t)nw : r0;
        CPROF_ADD(ta, 1);
        if (d <= m) return EMPTY_ID;
        CPROF_CNT(17, 1);
        st.E += d;
        const float dl = lane < d ? sp.dist[lane == pos ? d0 : lane] : -__int_as_float(0x7f800000);
        const bool nan = __ballot(lane < d && !(dl == dl)) != 0ull;
        float wm = dl;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) wm = fmaxf(wm, __shfl_xor(wm, o, 64));
        const unsigned long long at = __ballot(lane < d && dl == wm);
        if (!nan && __popcll(at) == 1) {  // a unique maximum: the map order is irrelevant
            worst = (uint32_t)guard_id(g, (uint32_t)__shfl(rv, __ffsll((long long)at) - 1, 64));
            worst_d = wm;
            decided = true;
        } else {
            load_query(q, g.vecs + (size_t)n * g.pitch);
            qn = g.norms[n];
        }
    } else {
        // n's row goes out with the append's loads (one round trip for both; most
        // appends overflow the row and evict)
        load_query(q, g.vecs + (size_t)n * g.pitch);
        qn = g.norms[n];
        d = list_append(g, l, n, nw, ev, &rv);
        CPROF_ADD(ta, 1);
        if (d <= m) return EMPTY_ID;
        CPROF_CNT(17, 1);
        st.E += d;
    }
    uint32_t nb = lane < d ? guard_id(g, (uint32_t)rv) : 0xFFFFFFFFu;
    if (!decided) {
        // graph.go:60-71 takes the first maximum in map order.  A unique maximum and
        // no NaN make the order irrelevant: score the row as it lies, and rank it
        // by key (the map-order stand-in) only when a tie or a NaN needs it.
        int nmax = 0;
        bool nan = false;
        if (!have_sp) {
            ev.template run<C, G>(g, q, qn, nb, d, g.metric, [&](float dd, uint32_t u) {
                nan |= !(dd == dd);
                if (dd > worst_d || worst == EMPTY_ID) {
                    worst_d = dd;
                    worst = u;
                    nmax = 1;
                } else if (dd == worst_d) {
                    ++nmax;
                }
            });
        }
        if (have_sp || nan || nmax > 1) {
            int64_t key = lane < d ? g.keys[nb] : INT64_MAX;
            rank_sort(key, nb, d);  // Go map order -> ascending key
            worst_d = -__int_as_float(0x7f800000);
            worst = EMPTY_ID;
            st.E += d;
            ev.template run<C, G>(g, q, qn, nb, d, g.metric, [&](float dd, uint32_t u) {  // graph.go:60-71
                if (dd > worst_d || worst == EMPTY_ID) {
                    worst_d = dd;
                    worst = u;
                }
            });
        }
    }
    CPROF_ADD(ta, 2);
    if (worst == EMPTY_ID) return EMPTY_ID;
    {
        int dd = d;
        list_remove_in(g, l, n, rv, dd, worst, ev);  // graph.go:74 (n's row is in registers since the append)
    }
    // worst's row, read after that removal (worst may be n itself)
    int32_t wrow = lane < capl ? ld_i32<true>(g.layers[l].adj + (size_t)worst * capl + lane) : -1;
    int wdeg = uni(ld_i32<true>(g.layers[l].deg + worst));
    if (wdeg >= 0) list_remove_in(g, l, worst, wrow, wdeg, n, ev);  // graph.go:76-78
    CPROF_ADD(ta, 3);
    replenish<C, G>(g, l, worst, m, S, st, err, ev, &wrow, wdeg);  // graph.go:79
    CPROF_ADD(ta, 4);
    return worst;
}

// Stage EvictSpec for add_neighbor(c_j, nw), j < cnt (lane j of nbh: c_j): the
// rows as they stand now, and one MW_PAIRS batch of every entry's distance to
// its row's owner plus nw's.  False when the staging area is too small (then
// every pair takes the plain path).
template <class C, int G, class Ev>
__device__ __forceinline__ bool stage_evictions(const GraphDev& g, int l, uint32_t nbh, int cnt, uint32_t nw,
                                                BuildSmem& S, const Ev& ev) {
    const int lane = lane_id();
    const int capl = g.layers[l].cap;
    if (!S.prow || cnt > S.pgroups || capl + 1 > S.pstride || cnt <= 0) return false;
    const int ps = S.pstride;
    const int tot = cnt * capl;
    for (int e0 = 0; e0 < tot; e0 += 64) {  // uniform trip count: the shuffles see every lane
        const int e = e0 + lane;
        const int j = min(e / capl, 63), i = e % capl;
        const uint32_t c = shfl_u(nbh, j);
        if (e < tot) S.prow[j * ps + i] = ld_i32<true>(g.layers[l].adj + (size_t)c * capl + i);
    }
    const int dj = lane < cnt ? ld_i32<true>(g.layers[l].deg + guard_id(g, nbh)) : -1;  // lane j: c_j's degree
    if (lane < cnt) S.pdeg[lane] = dj;
    ev.sync();
    // the pairs table: entries of row j (past its degree: none), then nw
    for (int e0 = 0; e0 < cnt * ps; e0 += 64) {
        const int e = e0 + lane;
        const int j = min(e / ps, 63), i = e % ps;
        const int djj = __shfl(dj, j, 64);
        const int dd = djj < 0 ? 0 : min(djj, capl);
        if (e < cnt * ps && i < dd) ev.pc[e] = (int32_t)guard_id(g, (uint32_t)S.prow[j * ps + i]);
        if (e < cnt * ps && i == dd) ev.pc[e] = (int32_t)nw;
    }
    if (lane < cnt) {
        ev.pq[lane] = nbh;
        ev.pn[lane] = (dj < 0 ? 0 : min(dj, capl)) + 1;
    }
    ev.sync();
    ev.template pairs<C, G>(g, cnt, g.metric);
    return true;
}

// graph.go:221-235 isolate: neighbours in ascending key order (the map-order
// stand-in) drop their backlink and are replenished; the deleted node's own
// row stays (the reference keeps the layerNode behind one-directional edges).
template <class C, int G, class Ev>
__device__ __forceinline__ void isolate(const GraphDev& g, int l, uint32_t n, int m, BuildSmem& S, WaveStats& st, int& err,
                        const Ev& ev) {
    const int lane = lane_id();
    const int capl = g.layers[l].cap;
    const int dn = min(uni(ld_i32<true>(g.layers[l].deg + n)), capl);
    if (dn < 0) return;  // nil neighbour map
    uint32_t mine = 0xFFFFFFFFu;
    int64_t key = INT64_MAX;
    if (lane < dn) {
        mine = guard_id(g, (uint32_t)ld_i32<true>(g.layers[l].adj + (size_t)n * capl + lane));
        key = g.keys[mine];
    }
    rank_sort(key, mine, dn);
    for (int j = 0; j < dn; ++j) {
        const uint32_t x = rl_u(mine, j);
        int32_t xrow = lane < capl ? ld_i32<true>(g.layers[l].adj + (size_t)x * capl + lane) : -1;
        int xdeg = uni(ld_i32<true>(g.layers[l].deg + x));
        if (xdeg < 0) continue;                            // neighbor.neighbors == nil
        list_remove_in(g, l, x, xrow, xdeg, n, ev);        // graph.go:232 delete(neighbor.neighbors, n.Key)
        replenish<C, G>(g, l, x, m, S, st, err, ev, &xrow, xdeg);  // graph.go:232
    }
}

// ---- multi-wave evaluator ----------------------------------------------------
// Protocol block in LDS.  The master posts a batch (query registers, ids,
// metric) and hits a workgroup barrier; every wave scores its share of the
// rows into dist[]; a second barrier hands the distances back.  Workers sit in
// mw_worker's loop between the two barriers until the master posts EXIT.
struct MwHdr {
    int cmd, cnt, metric;
    float qn;
};
constexpr int MW_EVAL = 0, MW_EXIT = 1, MW_PAIRS = 2;

// Everything exchanged here lives in LDS (workers read only immutable rows from
// HBM), so the fences order LDS alone: the master's graph stores are not waited
// for at every hand-off.
__device__ __forceinline__ void mw_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// rows [0, cnt) of ids, wave w of nw: canonical distances into dist[]
template <class C, int G>
__device__ __forceinline__ void mw_share(const GraphDev& g, const QReg<C>& q, float qn, const uint32_t* ids,
                                         float* dist, int cnt, int metric, int w, int nw) {
    using RM = RowMap<C, G>;
    constexpr int GROUP = C::LPR >> RM::LG;
    const int lane = lane_id();
    for (int base = w * RM::T; base < cnt; base += nw * RM::T) {
        uint32_t rid[G];
        bool valid[G];
#pragma unroll
        for (int gg = 0; gg < G; ++gg) {
            const int t = base + RM::reg_row(gg, lane);
            valid[gg] = t < cnt;
            rid[gg] = valid[gg] ? guard_id(g, ids[t]) : 0u;
        }
        const float s = metric == EUCLIDEAN ? eval_rows<C, G, true>(q, g.vecs, g.pitch, rid, valid)
                                            : eval_rows<C, G, false>(q, g.vecs, g.pitch, rid, valid);
        const int town = base + RM::owned_row(lane);
        if (town < cnt && (lane & (GROUP - 1)) == 0) {
            const float xn = metric == COSINE ? g.norms[guard_id(g, ids[town])] : 1.f;
            dist[town] = finalize(metric, s, xn, qn);
        }
    }
}

template <class C>
struct MwEval {
    static constexpr bool kPairs = true;
    MwHdr* hdr;
    float4* qbuf;     // [VPL * 64] the master's query registers, lane-major
    uint32_t* list;   // ids of the posted batch (also replenish's candidate list)
    float* dist;      // [cap] distances back
    int nw;
    // MW_PAIRS: group j scores rows pc[j * ps, + pn[j]) against row pq[j] into pd
    uint32_t* pq = nullptr;
    int* pn = nullptr;
    int32_t* pc = nullptr;
    float* pd = nullptr;
    int ps = 0;
    template <class C2, int G, class Sink>
    __device__ __forceinline__ void run_list(const GraphDev& g, const QReg<C2>& q, float qn, int cnt, int metric,
                                             Sink&& sink, bool sinks = true) const {
        if (cnt <= 0) return;
        const int lane = lane_id();
#pragma unroll
        for (int v = 0; v < C2::VPL; ++v) qbuf[v * 64 + lane] = q.v[v];
        if (lane == 0) {
            hdr->cmd = MW_EVAL;
            hdr->cnt = cnt;
            hdr->metric = metric;
            hdr->qn = qn;
        }
        CPROF_T(tp);
        mw_barrier();  // post
        mw_share<C2, G>(g, q, qn, list, dist, cnt, metric, 0, nw);
        mw_barrier();  // collect
        CPROF_ADD(tp, 11);
        // the results go through registers: the sink loop reads lanes, not LDS
        for (int b = 0; sinks && b < cnt; b += 64) {
            const int c = min(64, cnt - b);
            const float dv = lane < c ? dist[b + lane] : 0.f;
            const uint32_t iv = lane < c ? list[b + lane] : 0u;
            for (int t = 0; t < c; ++t) sink(rl_f(dv, t), rl_u(iv, t));
        }
        CPROF_ADD(tp, 12);
    }
    template <class C2, int G, class Sink>
    __device__ __forceinline__ void run(const GraphDev& g, const QReg<C2>& q, float qn, uint32_t cid, int cnt,
                                        int metric, Sink&& sink) const {
        if (cnt <= 0) return;
        if (lane_id() < cnt) list[lane_id()] = cid;
        run_list<C2, G>(g, q, qn, cnt, metric, sink);
    }
    // rows list[0, cnt): distance e into outd[e], the row into outi[e]
    template <class C2, int G>
    __device__ __forceinline__ void score(const GraphDev& g, const QReg<C2>& q, float qn, int cnt, int metric,
                                          float* outd, uint32_t* outi) const {
        run_list<C2, G>(g, q, qn, cnt, metric, [](float, uint32_t) {}, false);
        for (int e = lane_id(); e < cnt; e += 64) {
            outd[e] = dist[e];
            outi[e] = list[e];
        }
    }
    // every group j of the posted pairs table scored by the waves (pq / pn / pc
    // written by the caller), distances into pd
    template <class C2, int G>
    __device__ __forceinline__ void pairs(const GraphDev& g, int ngroups, int metric) const;
    // the master's own lanes only (workers never touch graph state)
    __device__ __forceinline__ void sync() const { wave_sync(); }
};

// MW_PAIRS, wave w of nw: whole groups j = w, w + nw, ... (each group's rows
// against its own owner row, loaded here)
template <class C, int G>
__device__ __forceinline__ void mw_pairs_share(const GraphDev& g, const MwEval<C>& ev, int ngroups, int metric, int w,
                                               int nw) {
    for (int j = w; j < ngroups; j += nw) {
        const uint32_t o = guard_id(g, uni(ev.pq[j]));
        QReg<C> q;
        load_query(q, g.vecs + (size_t)o * g.pitch);
        mw_share<C, G>(g, q, g.norms[o], reinterpret_cast<const uint32_t*>(ev.pc) + (size_t)j * ev.ps,
                       ev.pd + (size_t)j * ev.ps, uni(ev.pn[j]), metric, 0, 1);
    }
}

template <class C, int G>
__device__ __forceinline__ void mw_worker(const GraphDev& g, const MwEval<C>& ev, int w) {
    for (;;) {
        mw_barrier();
        const int cmd = ev.hdr->cmd;
        if (cmd == MW_EXIT) break;
        if (cmd == MW_PAIRS) {
            mw_pairs_share<C, G>(g, ev, ev.hdr->cnt, ev.hdr->metric, w, ev.nw);
        } else {
            QReg<C> q;
            const int lane = lane_id();
#pragma unroll
            for (int v = 0; v < C::VPL; ++v) q.v[v] = ev.qbuf[v * 64 + lane];
            mw_share<C, G>(g, q, ev.hdr->qn, ev.list, ev.dist, ev.hdr->cnt, ev.hdr->metric, w, ev.nw);
        }
        mw_barrier();
    }
}

template <class C>
template <class C2, int G>
__device__ __forceinline__ void MwEval<C>::pairs(const GraphDev& g, int ngroups, int metric) const {
    if (ngroups <= 0) return;
    if (lane_id() == 0) {
        hdr->cmd = MW_PAIRS;
        hdr->cnt = ngroups;
        hdr->metric = metric;
    }
    mw_barrier();  // post
    mw_pairs_share<C, G>(g, *this, ngroups, metric, 0, nw);
    mw_barrier();  // collect
}

// The sequential kernels re-read a layer's descriptor (row cap, adjacency and
// degree arrays) at every step of the walk; from HBM each read is one more
// dependent round trip (vector loads: the walk's own stores could alias the
// table, so the scalar cache is out).  A copy in LDS makes it a few dozen
// cycles.  Returns the graph view to walk with.
__device__ __forceinline__ GraphDev lds_layers(const GraphDev& g, LayerDev* tab) {
    for (int i = threadIdx.x; i < g.nlayers; i += blockDim.x) tab[i] = g.layers[i];
    __syncthreads();
    GraphDev v = g;
    v.layers = tab;
    return v;
}

// LDS of the compat walks: visited set, compat heaps, replenish heap + staging
__device__ __forceinline__ uint32_t* build_smem(uint32_t* p, int vis_log2, int M, int ef, BuildSmem& S) {
    S.cs.vis = p;
    S.cs.vlog2 = vis_log2;
    p += 1 << vis_log2;
    S.cs.cd = reinterpret_cast<float*>(p);
    p += ef + 2;
    S.cs.ci = p;
    p += ef + 2;
    S.cs.rd = reinterpret_cast<float*>(p);
    p += M + 2;
    S.cs.ri = p;
    p += M + 2;
    const int hcap = (M + 1) * (M + 1) + 2;  // >= any neighbours-of-neighbours list
    S.hcap = hcap;
    S.hd = reinterpret_cast<float*>(p);
    p += hcap;
    S.hi = p;
    p += hcap;
    S.radj = p;
    p += hcap;
    p += (reinterpret_cast<uintptr_t>(p) & 4) ? 1 : 0;  // 8-B align
    S.rkey = reinterpret_cast<int64_t*>(p);
    p += 2 * hcap;
    return p;
}
__host__ __device__ constexpr size_t build_smem_words(int vis_log2, int M, int ef) {
    return ((size_t)1 << vis_log2) + 2 * (size_t)(ef + 2) + 2 * (size_t)(M + 2) + 5 * (size_t)((M + 1) * (M + 1) + 2) + 1;
}

// One insert of graph.go:942-1042 (BatchAdd; Add is the same walk), by the
// master wave.  Rows: id_a for the layers above i0, id_b from i0 down (the same
// row for a fresh key).  ent[l]: the layer's entry() at its turn, or the
// inserted row itself when the layer is empty then (graph.go:990-993).  i0 >= 0
// (a present key, graph.go:1015-1024): after layer i0's search every layer
// holding the key deletes and isolates it (sweep[l], ascending), and the key's
// live row becomes id_b.  Returns false on the reference's "no nodes found in
// neighborhood search" (layer in *fail_layer).
template <class C, int G, class Ev>
__device__ __forceinline__ bool compat_insert(const CompatBuildArgs& a, BuildSmem& S, const Ev& ev, WaveStats& st, int& err,
                              int level, int top, uint32_t id_a, uint32_t id_b, int i0, const int32_t* ent,
                              const int32_t* sweep, int& fail_layer) {
    const int lane = lane_id();
    QReg<C> q;
    load_query(q, a.g.vecs + (size_t)id_b * a.g.pitch);
    const float qn = a.g.norms[id_b];
    uint32_t elevator = EMPTY_ID;
    for (int l = top; l >= 0; --l) {  // graph.go:980
        const uint32_t id = l > i0 ? id_a : id_b;
        if (ent[l] == (int32_t)id) {  // graph.go:990-993: empty layer, no search
            ev.sync();
            if (lane == 0) st_i32(a.g.layers[l].deg + id, -1);
            ev.sync();
            continue;
        }
        // graph.go:997-1003: layer.nodes[*elevator] -- nil once that key has no node here
        uint32_t sp = ent[l] < 0 ? EMPTY_ID : (uint32_t)ent[l];
        if (elevator != EMPTY_ID) sp = resolve_member<true>(a.g, l, elevator);
        int cnt = 0;
        CPROF_T(ts);
        if (sp != EMPTY_ID) cnt = compat_layer<C, G, true>(a.g, l, sp, a.M, a.ef, q, qn, S.cs, st, err, ev);  // :1005
        CPROF_ADD(ts, 0);
        if (cnt == 0) {  // search(nil) -> "no nodes found in neighborhood search"
            fail_layer = l;
            return false;
        }
        elevator = S.cs.ri[0];  // graph.go:1013
        if (level >= l) {       // graph.go:1015-1032
            const uint32_t nbh = lane < cnt ? S.cs.ri[lane] : 0u;
            if (l == i0) {
                CPROF_T(ti);
                for (int l2 = 0; l2 < a.g.nlayers; ++l2)  // graph.go:1018-1023
                    if (sweep[l2] >= 0) isolate<C, G>(a.g, l2, (uint32_t)sweep[l2], a.M, S, st, err, ev);
                ev.sync();
                if (lane == 0) st_i32(a.g.kidlive + kid_of(a.g, id_b), (int32_t)id_b);
                CPROF_ADD(ti, 10);
            }
            ev.sync();
            if (lane == 0) st_i32(a.g.layers[l].deg + id, -1);
            ev.sync();
            CPROF_T(tn);
            // Eviction speculation: the neighbourhood's rows and their distances
            // are staged in one batch; pair j uses them unless an earlier pair of
            // this loop changed c_j's row -- which only an eviction of c_j does
            // (an addNeighbor pair writes its own two rows, and the evicted row
            // with its replenish): then it reads the row as usual.
            bool staged = false;
            if constexpr (Ev::kPairs) staged = stage_evictions<C, G>(a.g, l, nbh, cnt, id, S, ev);
            uint32_t evicted = EMPTY_ID;  // lane k: the k-th row evicted in this loop
            int nev = 0;
            for (int j = 0; j < cnt; ++j) {
                const uint32_t c = rl_u(nbh, j);
                const bool fresh = staged && nev < 64 && __ballot(lane < nev && evicted == c) == 0ull;
                // the staged row is read only when fresh (S.pdeg / S.prow are null without staging)
                const EvictSpec sp = fresh ? EvictSpec{S.prow + j * S.pstride, uni(S.pdeg[j]), S.pdist + j * S.pstride}
                                           : EvictSpec{nullptr, 0, nullptr};
                const uint32_t w1 = add_neighbor<C, G>(a.g, l, c, id, a.M, S, st, err, ev, fresh, sp);
                if (w1 != EMPTY_ID) {
                    if (lane == nev) evicted = w1;
                    ++nev;
                }
                const uint32_t w2 = add_neighbor<C, G>(a.g, l, id, c, a.M, S, st, err, ev);
                if (w2 != EMPTY_ID) {
                    if (lane == nev) evicted = w2;
                    ++nev;
                }
            }
            CPROF_ADD(tn, 13);
        }
    }
    return true;
}

// graph.go:942-1042 for the fresh inserts [n0, n1), then the replacing insert
// (a.rep_level >= 0), in order; the first failing insert ends the walk
template <class C, int G, class Ev>
__device__ __forceinline__ void compat_inserts(const CompatBuildArgs& a, BuildSmem& S, const Ev& ev, WaveStats& st, int& err) {
    int top = a.top0;
    int fail_layer = -1;
    int64_t fail_row = -1;
    for (int64_t i = a.n0; i < a.n1; ++i) {
        const uint32_t id = (uint32_t)i;
        const int level = a.levels[i];
        top = max(top, level);
        if (!compat_insert<C, G>(a, S, ev, st, err, level, top, id, id, -1, a.layer_entry, a.rep_sweep,
                                 fail_layer)) {
            fail_row = i;
            break;
        }
        if (err) break;
    }
    if (fail_row < 0 && !err && a.rep_level >= 0) {
        top = max(top, a.rep_level);
        if (!compat_insert<C, G>(a, S, ev, st, err, a.rep_level, top, a.rep_a, a.rep_b, a.rep_i0, a.rep_entry,
                                 a.rep_sweep, fail_layer))
            fail_row = a.rep_b;
    }
    if (fail_row >= 0) {
        err |= 2;
        if (lane_id() == 0) {
            a.err[2] = fail_layer;
            a.err[3] = (int)fail_row;
        }
    }
}

template <class C, int G>
__global__ __launch_bounds__(64) void k_build_compat(CompatBuildArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    __shared__ LayerDev ltab[MH_MAXL];
    a.g = lds_layers(a.g, ltab);
    BuildSmem S;
    uint32_t* p = build_smem(smem, a.vis_log2, a.M, a.ef, S);
    WaveEval ev;
    ev.list = p;
    WaveStats st;
    int err = 0;
    compat_inserts<C, G>(a, S, ev, st, err);
    if (lane_id() == 0) {
        atomicAdd(&a.stats[0], st.E);
        atomicAdd(&a.stats[1], st.X);
        if (err) atomicOr(a.err, err);
    }
}

// The same walk with distance batches spread over NW waves (the sequential
// insert is latency-bound: one wave keeps too few rows in flight).
template <class C, int G, int NW>
__global__ __launch_bounds__(64 * NW) void k_build_compat_mw(CompatBuildArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    __shared__ LayerDev ltab[MH_MAXL];
    a.g = lds_layers(a.g, ltab);
    BuildSmem S;
    uint32_t* p = build_smem(smem, a.vis_log2, a.M, a.ef, S);
    MwEval<C> ev;
    p += (4 - (reinterpret_cast<uintptr_t>(p) >> 2) % 4) % 4;  // 16-B align: qbuf is read/written as float4
    ev.hdr = reinterpret_cast<MwHdr*>(p);
    p += 4;
    ev.qbuf = reinterpret_cast<float4*>(p);
    p += 4 * 64 * C::VPL;
    ev.list = p;
    p += S.hcap;
    ev.dist = reinterpret_cast<float*>(p);
    p += S.hcap;
    ev.nw = NW;
    // eviction speculation staging (stage_evictions): M groups of M + 2, when
    // the launch found room for it
    S.pgroups = a.spec ? a.M : 0;
    S.pstride = a.M + 2;
    const int pt = S.pgroups * S.pstride;
    S.prow = a.spec ? reinterpret_cast<int32_t*>(p) : nullptr;
    p += pt;
    // without staging (large M: the launch found no room) every staging pointer
    // stays null -- they lie past the dynamic LDS allocation
    ev.pc = a.spec ? reinterpret_cast<int32_t*>(p) : nullptr;
    p += pt;
    ev.pd = a.spec ? reinterpret_cast<float*>(p) : nullptr;
    S.pdist = ev.pd;
    p += pt;
    S.pdeg = a.spec ? reinterpret_cast<int*>(p) : nullptr;
    p += 64;
    ev.pq = a.spec ? p : nullptr;
    p += 64;
    ev.pn = a.spec ? reinterpret_cast<int*>(p) : nullptr;
    ev.ps = S.pstride;
    const int wave = threadIdx.x >> 6;
    if (wave != 0) {
        mw_worker<C, G>(a.g, ev, wave);
        return;
    }
    WaveStats st;
    int err = 0;
#ifdef MH_COMPAT_PROF
    if (lane_id() < 24) mh_cprof[lane_id()] = 0;
    __builtin_amdgcn_wave_barrier();
    CPROF_T(tk);
    CPROF_CNT(16, a.n1 - a.n0);
#endif
    compat_inserts<C, G>(a, S, ev, st, err);
#ifdef MH_COMPAT_PROF
    CPROF_ADD(tk, 21);
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    if (lane_id() == 0) {
        for (int i = 0; i < 24; ++i) printf("cprof %d %llu\n", i, mh_cprof[i]);
    }
#endif
    if (lane_id() == 0) ev.hdr->cmd = MW_EXIT;
    mw_barrier();  // releases the workers
    if (lane_id() == 0) {
        atomicAdd(&a.stats[0], st.E);
        atomicAdd(&a.stats[1], st.X);
        if (err) atomicOr(a.err, err);
    }
}

// ---------------------------------------------------------------------------
// delete (graph.go:843-895)
// ---------------------------------------------------------------------------
// Delete / BatchDelete with the reference's semantics: one wave walks the keys
// in order and every layer holding the node (graph.go:852-861).
template <class C, int G>
__global__ __launch_bounds__(64) void k_delete_compat(DeleteArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    __shared__ LayerDev ltab[MH_MAXL];
    a.g = lds_layers(a.g, ltab);
    const int lane = lane_id();
    BuildSmem S;
    uint32_t* p = build_smem(smem, a.vis_log2, a.M, 0, S);
    WaveEval ev;
    ev.list = p;
    WaveStats st;
    int err = 0;
    for (int64_t i = 0; i < a.nids; ++i) {
        const uint32_t id = a.ids[i];
        const int l = (int)a.lay[i];
        if (uni(ld_i32<true>(a.g.layers[l].deg + id)) == -2) continue;
        isolate<C, G>(a.g, l, id, a.M, S, st, err, ev);
    }
    if (lane == 0) {
        atomicAdd(&a.stats[0], st.E);
        if (err) atomicOr(a.err, err);
    }
}

constexpr int MW_WAVES = 8;
// dynamic LDS a sequential kernel may ask for: 160 KiB less its static layer
// table (and the tools-only counters)
constexpr size_t CW_LDS_MAX = 160 * 1024 - MH_MAXL * sizeof(LayerDev) - 256;

template <int L, int V>
int launch_build_compat_cfg(const CompatBuildArgs& a, int waves, hipStream_t s) {
    using C = Cfg<L, V>;
    // the sequential build keeps three query rows live (search / addNeighbor /
    // replenish): up to 4 rows in flight per group to 768-d, 2 above (spill-free)
    constexpr int G = std::min(cfg_group<L, V>(), V <= 3 ? 4 : 2);
    const size_t base = build_smem_words(a.vis_log2, a.M, a.ef);
    const int hcap = (a.M + 1) * (a.M + 1) + 2;
    if (waves <= 1 || C::VPL >= 16) {  // 4096-d: the walking wave alone (register budget)
        const size_t lds = (base + hcap) * 4;
        if (lds > CW_LDS_MAX) return -2;
        hipLaunchKernelGGL((k_build_compat<C, G>), dim3(1), dim3(64), lds, s, a);
    } else {
        const size_t spec = 3 * (size_t)a.M * (a.M + 2) + 3 * 64;  // eviction speculation staging
        const size_t core = (base + 3 + 4 + 4 * 64 * (size_t)C::VPL + 2 * (size_t)hcap) * 4;
        CompatBuildArgs b = a;
        b.spec = core + spec * 4 <= CW_LDS_MAX ? 1 : 0;  // large M: no staging (same graph)
        const size_t lds = core + (b.spec ? spec * 4 : 0);
        if (lds > CW_LDS_MAX) return -2;
        hipLaunchKernelGGL((k_build_compat_mw<C, G, MW_WAVES>), dim3(1), dim3(64 * MW_WAVES), lds, s, b);
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

template <int L, int V>
int launch_delete_compat_cfg(const DeleteArgs& a, hipStream_t s) {
    constexpr int G = std::min(cfg_group<L, V>(), 2);  // the insert's narrower width, at every dimension
    const size_t words = build_smem_words(a.vis_log2, a.M, 0) + (size_t)((a.M + 1) * (a.M + 1) + 2);
    if (words * 4 > CW_LDS_MAX) return -2;
    hipLaunchKernelGGL((k_delete_compat<Cfg<L, V>, G>), dim3(1), dim3(64), words * 4, s, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace mh
