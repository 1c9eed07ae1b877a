// build_batch.hpp -- the throughput insert and the repair delete, instantiated
// per configuration in build_units.hip.  A batch of new nodes is searched in
// parallel against the graph as it stood before the batch (k_batch_search: one
// wave per node, beam search with efConstruction), each node selects its
// neighbours and writes its own row; reverse edges are proposed into per-target
// slots and committed by one wave per touched node (k_batch_commit), keeping the
// best cap by (distance, id) -- graph.go:55-80 generalised to a set of
// proposals, independent of arrival order.  k_delete_repair selects the same way.
#pragma once
#include <algorithm>
#include <type_traits>

#include "device_search.hpp"
#include "engine.hpp"

namespace mh {

template <int L, int V>
int launch_batch_descend_cfg(const BatchBuildArgs& a, hipStream_t s);
// XW: entries expanded per step of the layer search (option "build_expand", 1-4)
template <int L, int V, int XW>
int launch_batch_search_cfg(const BatchBuildArgs& a, hipStream_t s);
template <int L, int V>
int launch_batch_commit_cfg(const BatchBuildArgs& a, int64_t max_touched, hipStream_t s);
template <int L, int V>
int launch_delete_repair_cfg(const DeleteArgs& a, hipStream_t s);

// ---------------------------------------------------------------------------
// batched build
// ---------------------------------------------------------------------------
// One kept row r (f32 row qr, norm rn) applied to every candidate still
// standing after list position pos (entry e = k * 64 + lane of the NR
// registers: bit k of live / dropped, id ids[k] & ID_MASK, d(u, c) ed[k] --
// the list's own registers, nothing copied): a candidate is dropped
// when alpha d(c, r) < d(u, c) -- decided by a two-sided screen of the
// candidates' fp16 rows against per-row thresholds, the undecided pairs in
// f32 (the neighbour selection of k_batch_search and k_batch_commit).
template <class C, int G, int NR>
__device__ __forceinline__ void drop_pass(const GraphDev& g, const QReg<C>& qr, float rn, int pos,
                                          uint32_t live, uint32_t& dropped, const uint32_t (&ids)[NR],
                                          const float (&ed)[NR], float alpha, float margin, WaveStats& st) {
    const int lane = lane_id();
    const bool scr = h16_query_ok(rn);
    st.F += 1;  // the kept row
    // (the body is too large to unroll: register r's id / distance are picked by
    // a small unrolled select, which keeps the list's registers out of scratch)
    for (int r = 0; r < NR; ++r) {
        uint32_t idr = ids[0];
        float edr = ed[0];
#pragma unroll
        for (int k = 1; k < NR; ++k) {  // bitwise selects: a `?:` chain is folded back into an indexed load
            const uint32_t mk = k == r ? 0xFFFFFFFFu : 0u;
            idr = (ids[k] & mk) | (idr & ~mk);
            edr = bsel(mk, ed[k], edr);
        }
        const bool cand = ((live & ~dropped) >> r & 1u) && r * 64 + lane >= pos;
        const unsigned long long m = __ballot(cand);
        if (!m) continue;
        const int cnt = __popcll(m);
        const int before =
            __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0));
        const int dst = cand ? before : cnt + (lane - before);
        const uint32_t cc = push_to(idr & ID_MASK, dst);
        const float cd = __uint_as_float(push_to(__float_as_uint(edr), dst));
        st.E += cnt;
        // with t = d(u, c) / alpha: an estimate proving d(c, r) > t (1 + 2^-20)
        // keeps c, one proving d(c, r) < t (1 - 2^-20) drops it; the brackets
        // absorb the roundings of t and of the rule's product, so
        // fl(alpha d) >= d(u, c) above and < below
        const float t = cd / alpha;
        int cls = 0;
        if (scr) {
            cls = screen_pairs<C, G>(g, qr, rn, cc, cnt, g.metric, t * (1.0f - 0x1p-20f),
                                     t * (1.0f + 0x1p-20f), margin);
            st.S += cnt;
        }
        if (!(cd > 0.f)) cls = 0;  // as the candidate-major loop: no screen for d(u, c) <= 0
        bool dr = lane < cnt && cls < 0;
        const bool und = lane < cnt && cls == 0;
        const unsigned long long mu = __ballot(und);
        if (mu) {
            const int nu = __popcll(mu);
            const int bu =
                __builtin_amdgcn_mbcnt_hi((uint32_t)(mu >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mu, 0));
            const int du = und ? bu : nu + (lane - bu);
            const uint32_t cu = push_to(cc, du);
            const float dcu = __uint_as_float(push_to(__float_as_uint(cd), du));
            st.F += nu;
            bool dk = false;
            int k = 0;
            eval_list<C, G>(g, qr, rn, cu, nu, g.metric, [&](float dcs, uint32_t) {
                const bool drop = alpha * dcs < rl_f(dcu, k);
                if (lane == k) dk = drop;
                ++k;
            });
            const int dks = __shfl((int)dk, du, 64);  // all lanes: a shuffle reads inactive lanes as 0
            dr = dr || (und && dks != 0);
        }
        const int drs = __shfl((int)dr, dst, 64);
        if (cand && drs != 0) dropped |= 1u << r;
    }
}

// the insert searches' visited set: 2^vis_log2 32-bit entries, or (vis16) the
// compact set -- 8,192 ids in 16 KiB where 2^12 entries held 4,096 (fewer
// resets, fewer re-evaluated candidates; the same lists, so the same graph)
__device__ __forceinline__ int batch_vsize(const BatchBuildArgs& a) { return a.vis16 ? -1 : 1 << a.vis_log2; }
__host__ __device__ inline int batch_vis_words(const BatchBuildArgs& a) {
    return a.vis16 ? std::max(1 << a.vis_log2, VIS16_WORDS) : 1 << a.vis_log2;
}

// Greedy descent (ef = 1) of every new node through the layers above its own
// level, all layers in one launch.  Every layer l is read before its commit
// (run_batch_layers commits layer l only after this kernel), exactly what the
// per-layer descent inside k_batch_search reads, so the graph is the same.
template <class C, int G, bool SCREEN>
__global__ __launch_bounds__(64) void k_batch_descend(BatchBuildArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    const int64_t u64 = a.n0 + blockIdx.x;
    if (u64 >= a.n1) return;
    const uint32_t u = a.rows ? a.rows[u64] : (uint32_t)u64;  // (the row-list form: BatchBuildArgs::rows)
    const int lv = a.levels[u];
    if (lv >= a.layer) return;
    WaveStats st;
    QReg<C> q;
    load_query(q, a.g.vecs + (size_t)u * a.g.pitch);
    const float qn = a.g.norms[u];
    uint32_t ep = a.cur_entry[u];
    for (int l = a.layer; l > lv; --l) {
        BList<1> L1;
        beam_layer<C, 1, G, false, SCREEN>(a.g, l, ep, 1, q, qn, L1, smem, batch_vsize(a), st);
        float d;
        uint32_t id;
        bl_at(L1, 0, d, id);
        if (id != EMPTY_ID) ep = id & ID_MASK;
    }
    if (lane_id() == 0) {
        a.cur_entry[u] = ep;
        atomicAdd(&a.stats[0], st.E);
        atomicAdd(&a.stats[1], st.X);
        atomicAdd(&a.stats[6], st.S);
        atomicAdd(&a.stats[7], st.F);
    }
}

// The neighbour selection of one row from its candidate list L (the first nl
// entries, ranked by (distance, id)): up to a.mcap live candidates, by HNSW's
// diversity rule when a.heuristic is set (a.alpha its slack), then
// a.keep_pruned's fill.  Lane j < the count returned holds the j-th neighbour
// in sel / seld.  Used by the insert (batch_insert) and by the link pass
// (build_link.hpp k_batch_link).
template <class C, int R, int G, bool SCREEN>
__device__ __forceinline__ int select_neighbours(const BatchBuildArgs& a, const BList<R>& L, int nl, uint32_t& sel,
                                                 float& seld, WaveStats& st) {
    const int lane = lane_id();
    bool sel_screen = false;
    float margin = 0.f;
    if constexpr (SCREEN) {
        sel_screen = a.g.h16 != nullptr && a.alpha > 0.f;
        const float e = a.g.h16err ? *a.g.h16err : 0.00048828125f;
        margin = a.g.metric == EUCLIDEAN ? h16_margin_l2(e) : h16_margin_cos(e);
    }
    int nsel = 0;
    // Screened: the same rule applied kept-row-major.  A candidate is kept
    // iff no kept row before it drops it, so each kept row r can be applied
    // at once to every later candidate still standing (one batched
    // two-sided screen of their fp16 rows, r's f32 row the query, and the
    // undecided pairs in f32); the next candidate standing is kept.
    // d(c, r) == d(r, c) bitwise (commutative products, norms multiplied
    // both ways round), so every decision is the candidate-major loop's
    // below (the unscreened path): the same graph (test_gpu_screen.py
    // compares with screen 0).  A candidate meets kept rows only until the
    // first one drops it, and the kept rows, not the candidates, are read
    // in f32: 15.4k -> 10.0k pair evaluations and 1.38k -> 0.99k f32 rows
    // per insert on the bench index.
    const bool rowmajor = SCREEN && sel_screen && a.heuristic;
    if (rowmajor) {
        uint32_t live = 0u, dropped = 0u;  // bit r: entry r * 64 + lane
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (L.i[r] != EMPTY_ID && r * 64 + lane < nl && !is_dead(a.g, L.i[r] & ID_MASK)) live |= 1u << r;
        int pos = 0;
        while (nsel < a.mcap) {
            int idx = -1;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const unsigned long long m = __ballot(((live & ~dropped) >> r & 1u) && r * 64 + lane >= pos);
                if (idx < 0 && m) idx = r * 64 + __ffsll((long long)m) - 1;
            }
            if (idx < 0) break;
            float dc;
            uint32_t c;
            bl_at(L, idx, dc, c);
            c &= ID_MASK;
            if (lane == nsel) {
                sel = c;
                seld = dc;
            }
            ++nsel;
            pos = idx + 1;
            if (nsel >= a.mcap) break;
            QReg<C> qr;
            load_query(qr, a.g.vecs + (size_t)c * a.g.pitch);
            drop_pass<C, G, R>(a.g, qr, a.g.norms[c], pos, live, dropped, L.i, L.d, a.alpha, margin, st);
        }
    }
    for (int i = 0; !rowmajor && i < nl && nsel < a.mcap; ++i) {
        float dc;
        uint32_t c;
        bl_at(L, i, dc, c);
        if (c == EMPTY_ID) break;
        c &= ID_MASK;
        if (is_dead(a.g, c)) continue;
        bool good = true;
        if (a.heuristic && nsel > 0) {  // HNSW Alg. 4: drop c if closer to a kept neighbour than to u
            QReg<C> qc;
            load_query(qc, a.g.vecs + (size_t)c * a.g.pitch);
            const float cn = a.g.norms[c];
            st.E += nsel;
            auto rule = [&](float dcs, uint32_t) {
                if (a.alpha * dcs < dc) good = false;
            };
            st.F += nsel + 1;  // the candidate's row and the kept rows, in f32
            eval_list<C, G>(a.g, qc, cn, sel, nsel, a.g.metric, rule);
        }
        if (good) {
            if (lane == nsel) {
                sel = c;
                seld = dc;
            }
            ++nsel;
        }
    }
    if (a.keep_pruned && nsel < a.mcap) {  // Malkov Alg. 4 keepPrunedConnections
        for (int i = 0; i < nl && nsel < a.mcap; ++i) {
            float dc;
            uint32_t c;
            bl_at(L, i, dc, c);
            if (c == EMPTY_ID) break;
            c &= ID_MASK;
            if (is_dead(a.g, c)) continue;
            if (__ballot(lane < nsel && sel == c)) continue;
            if (lane == nsel) {
                sel = c;
                seld = dc;
            }
            ++nsel;
        }
    }
    return nsel;
}

#ifndef MH_BUILD_WPS
#define MH_BUILD_WPS 1
#endif
// One insert u of a batch at layer a.layer: greedy descent above u's level,
// else the layer search (efConstruction), the neighbour selection and the
// reverse proposals.  bev scores the search's candidate batches (WaveBatch:
// this wave; MwBatch: the workgroup's waves, k_batch_search_mw).
template <class C, int R, int G, bool SCREEN, int XW, class BEv>
__device__ __forceinline__ void batch_insert(const BatchBuildArgs& a, uint32_t u, const QReg<C>& q, float qn,
                                             uint32_t* smem, WaveStats& st, const BEv& bev) {
    const int lane = lane_id();
    const int l = a.layer;
    const uint32_t ep = a.cur_entry[u];
    if (a.levels[u] < l) {  // above the node's level: greedy descent only
        BList<1> L1;
        beam_layer<C, 1, G, false, SCREEN, 1>(a.g, l, ep, 1, q, qn, L1, smem, batch_vsize(a), st, bev);
        float d;
        uint32_t id;
        bl_at(L1, 0, d, id);
        if (lane == 0 && id != EMPTY_ID) a.cur_entry[u] = id & ID_MASK;
    } else {
        BList<R> L;
        // lists of 256 / 512 entries on the one-wave kernel merge each step's
        // candidates at once (bl_merge; scratch after the visited set, sized by
        // launch_batch_search_cfg)
        constexpr bool MRG = R >= 4 && std::is_same<BEv, WaveBatch>::value;
        float* mrg = MRG ? reinterpret_cast<float*>(smem + batch_vis_words(a)) : nullptr;
        beam_layer<C, R, G, false, SCREEN, XW, MRG>(a.g, l, ep, a.ef, q, qn, L, smem, batch_vsize(a), st, bev, mrg);
        float d0;
        uint32_t i0;
        bl_at(L, 0, d0, i0);
        if (lane == 0 && i0 != EMPTY_ID) a.cur_entry[u] = i0 & ID_MASK;
        // neighbour selection
        uint32_t sel = 0;
        float seld = 0.f;
        const int nsel = select_neighbours<C, R, G, SCREEN>(a, L, a.ef, sel, seld, st);
        const int capl = a.g.layers[l].cap;
        if (lane < nsel) {
            a.g.layers[l].adj[(size_t)u * capl + lane] = (int32_t)sel;
            a.g.layers[l].adjd[(size_t)u * capl + lane] = seld;
            const int slot = atomicAdd(&a.inc_cnt[sel], 1);
            if (slot < a.inc_cap) {
                a.inc_src[(size_t)sel * a.inc_cap + slot] = u;
                a.inc_dist[(size_t)sel * a.inc_cap + slot] = seld;
            } else {
                atomicAdd(&a.stats[2], 1ull);
            }
            if (slot == 0) {
                const int t = atomicAdd(a.touched_cnt, 1);
                a.touched[t] = sel;
            }
        }
        if (lane == 0) a.g.layers[l].deg[u] = nsel;
    }
}

__device__ __forceinline__ void batch_stats(const BatchBuildArgs& a, const WaveStats& st) {
    if (lane_id() == 0) {
        atomicAdd(&a.stats[0], st.E);
        atomicAdd(&a.stats[1], st.X);
        atomicAdd(&a.stats[6], st.S);
        atomicAdd(&a.stats[7], st.F);
    }
}

__device__ __forceinline__ bool batch_node(const BatchBuildArgs& a, uint32_t& u) {
    if (a.order) {
        if (blockIdx.x >= a.count) return false;
        u = a.order[blockIdx.x];
    } else {
        const int64_t u64 = a.n0 + blockIdx.x;
        if (u64 >= a.n1) return false;
        u = a.rows ? a.rows[u64] : (uint32_t)u64;
    }
    return true;
}

template <class C, int R, int G, bool SCREEN, int XW>
__global__ __launch_bounds__(64, MH_BUILD_WPS) void k_batch_search(BatchBuildArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    uint32_t u;
    if (!batch_node(a, u)) return;
    WaveStats st;
    QReg<C> q;
    load_query(q, a.g.vecs + (size_t)u * a.g.pitch);
    const float qn = a.g.norms[u];
    batch_insert<C, R, G, SCREEN, XW>(a, u, q, qn, smem, st, WaveBatch());
    batch_stats(a, st);
}

// Narrow launches (few inserts: the first batches of a build, the upper layers
// of every batch) leave most of the chip idle and each insert's ~550 dependent
// expansions on one wave: one workgroup of BMW_WAVES waves per insert splits
// every candidate batch over the waves (k_search_beam_mw's protocol).  Same
// graph as k_batch_search, bit for bit (the list keeps the best ef of what is
// inserted, whatever the order; the screen tests the pre-batch worst on every
// wave).
template <class C, int R, int G, bool SCREEN, int XW>
__global__ __launch_bounds__(64 * BMW_WAVES) void k_batch_search_mw(BatchBuildArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    __shared__ BmwShare sh;
    uint32_t u;
    if (!batch_node(a, u)) return;  // (whole workgroup)
    const int wave = threadIdx.x >> 6;
    WaveStats st;
    QReg<C> q;
    load_query(q, a.g.vecs + (size_t)u * a.g.pitch);
    const float qn = a.g.norms[u];
    if (wave == 0) {
        batch_insert<C, R, G, SCREEN, XW>(a, u, q, qn, smem, st, MwBatch{&sh});
        if (lane_id() == 0) sh.cmd = BMW_EXIT;
        bmw_barrier();  // releases the other waves
    } else {
        const bool screen = SCREEN && h16_query_ok(qn);
        float margin = 0.f;
        if constexpr (SCREEN) {
            const float e = a.g.h16err ? *a.g.h16err : 0.00048828125f;
            margin = a.g.metric == EUCLIDEAN ? h16_margin_l2(e) : h16_margin_cos(e);
        }
        for (;;) {
            bmw_barrier();
            if (sh.cmd == BMW_EXIT) break;
            st.F += bmw_share<C, G, SCREEN>(a.g, q, qn, &sh, wave, screen, margin, st.S);
            bmw_barrier();
        }
    }
    batch_stats(a, st);
}

// One wave per touched node v: merge v's row with the proposals it received.
// (existing U proposals) is ranked by (dist to v, id); when it fits the row it
// is written in rank order, otherwise the best `cap` are kept -- or, with
// heuristic >= 2, HNSW's diversity rule (Alg. 4) is applied on overflow: a
// candidate is dropped when it is closer to an already kept neighbour than to v.
template <class C, int G>
__global__ __launch_bounds__(64) void k_batch_commit(BatchBuildArgs a) {
    __shared__ float sd[128];
    __shared__ uint32_t si[128];
    __shared__ float rd[128];
    __shared__ uint32_t ri[128];
    const int lane = lane_id();
    const int n_t = *a.touched_cnt;
    // grid-stride over the touched rows: a bounded grid (at most 32,768
    // workgroups) instead of one workgroup per row the batch could touch (mcap
    // per insert: 8M for a 200k batch at M0 40, nearly all of which would only
    // read the count and exit)
    for (int t = blockIdx.x; t < n_t; t += gridDim.x) {
        const uint32_t v = a.touched[t];
        const int l = a.layer;
        const int capl = a.g.layers[l].cap;
        const int keep_cap = min(capl, a.mcap);
        int32_t* row = a.g.layers[l].adj + (size_t)v * capl;
        float* rowd = a.g.layers[l].adjd + (size_t)v * capl;
        int d = a.g.layers[l].deg[v];
        if (d < 0) d = 0;
        int nin = a.inc_cnt[v];
        if (nin > a.inc_cap) nin = a.inc_cap;
        const int tot = d + nin;
        for (int e = lane; e < 128; e += 64) {
            float dd = __int_as_float(0x7f800000);
            uint32_t ii = EMPTY_ID;
            if (e < d) {
                ii = (uint32_t)row[e];
                dd = rowd[e];
            } else if (e < tot) {
                ii = a.inc_src[(size_t)v * a.inc_cap + (e - d)];
                dd = a.inc_dist[(size_t)v * a.inc_cap + (e - d)];
            }
            sd[e] = dd;
            si[e] = ii;
        }
        __syncthreads();
        // rank = number of entries ordered before this one by (dist, id)
        for (int h = 0; h < 2; ++h) {
            const int e = lane + 64 * h;
            const float md = sd[e];
            const uint32_t mi = si[e];
            int rank = 0;
            for (int f = 0; f < tot; ++f) rank += lt_di(sd[f], si[f], md, mi) ? 1 : 0;
            if (e < tot) {
                rd[rank] = md;
                ri[rank] = mi;
            }
        }
        __syncthreads();
        int nkeep = 0;
        if (tot <= keep_cap || a.heuristic < 2) {
            nkeep = min(tot, keep_cap);
            for (int e = lane; e < nkeep; e += 64) {
                row[e] = (int32_t)ri[e];
                rowd[e] = rd[e];
            }
        } else {
            uint32_t kept = 0;   // lane j holds the j-th kept id
            float keptd = 0.f;
            WaveStats st;
            // with the fp16 copy: kept-row-major, as k_batch_search's selection
            // (drop_pass; the same decisions as the candidate-major loop below)
            const bool rowmajor = a.g.h16 != nullptr && a.alpha > 0.f;
            if (rowmajor) {
                const float e = a.g.h16err ? *a.g.h16err : 0.00048828125f;
                const float margin = a.g.metric == EUCLIDEAN ? h16_margin_l2(e) : h16_margin_cos(e);
                uint32_t live = 0u, dropped = 0u;
                uint32_t eid[2];
                float ed[2];
    #pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int e2 = lane + 64 * h;
                    if (e2 < tot) live |= 1u << h;
                    eid[h] = e2 < tot ? guard_id(a.g, ri[e2]) : 0u;
                    ed[h] = rd[e2];
                }
                int pos = 0;
                while (nkeep < keep_cap) {
                    int idx = -1;
    #pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const unsigned long long m = __ballot(((live & ~dropped) >> h & 1u) && h * 64 + lane >= pos);
                        if (idx < 0 && m) idx = h * 64 + __ffsll((long long)m) - 1;
                    }
                    if (idx < 0) break;
                    const uint32_t c = ri[idx];
                    if (lane == nkeep) {
                        kept = c;
                        keptd = rd[idx];
                    }
                    ++nkeep;
                    pos = idx + 1;
                    if (nkeep >= keep_cap) break;
                    QReg<C> qr;
                    const uint32_t cg = guard_id(a.g, c);
                    load_query(qr, a.g.vecs + (size_t)cg * a.g.pitch);
                    drop_pass<C, G, 2>(a.g, qr, a.g.norms[cg], pos, live, dropped, eid, ed, a.alpha, margin, st);
                }
            }
            for (int i = 0; !rowmajor && i < tot && nkeep < keep_cap; ++i) {
                const uint32_t c = ri[i];
                const float dcv = rd[i];
                bool good = true;
                if (nkeep > 0) {
                    QReg<C> qc;
                    load_query(qc, a.g.vecs + (size_t)guard_id(a.g, c) * a.g.pitch);
                    const float cn = a.g.norms[guard_id(a.g, c)];
                    st.E += nkeep;
                    st.F += nkeep + 1;  // the candidate's row and the kept rows, in f32
                    eval_list<C, G>(a.g, qc, cn, kept, nkeep, a.g.metric, [&](float dcs, uint32_t) {
                        if (a.alpha * dcs < dcv) good = false;
                    });
                }
                if (good) {
                    if (lane == nkeep) {
                        kept = c;
                        keptd = dcv;
                    }
                    ++nkeep;
                }
            }
            if (lane < nkeep) {
                row[lane] = (int32_t)kept;
                rowd[lane] = keptd;
            }
            if (lane == 0) {  // the pruning's rows count as the insert's reads (bench.py build roofline)
                atomicAdd(&a.stats[0], st.E);
                atomicAdd(&a.stats[6], st.S);
                atomicAdd(&a.stats[7], st.F);
            }
        }
        if (lane == 0) {
            a.g.layers[l].deg[v] = nkeep;
            a.inc_cnt[v] = 0;
        }
        __syncthreads();  // (the LDS rank arrays are reused by the next row)
    }
}

// Batched-graph repair, one wave per row of layer a.layer: a live row that
// points at a deleted node is rebuilt from its live neighbours plus the rows
// of its deleted neighbours (gather order, first REPAIR_POOL kept), ranked by
// (distance, id) and selected like k_batch_search (diversity heuristic,
// optional keep-pruned fill).  Deleted rows are only read and live rows are
// only written by their owner, so rows are independent.  Restated in
// oracle/oracle.c repair_layer.
template <class C, int G>
__global__ __launch_bounds__(64) void k_delete_repair(DeleteArgs a) {
    __shared__ uint32_t pid[REPAIR_POOL];
    __shared__ float pd[REPAIR_POOL];
    __shared__ uint32_t sid[REPAIR_POOL];
    __shared__ float sdd[REPAIR_POOL];
    const int64_t v64 = blockIdx.x;
    if (v64 >= a.n) return;
    const uint32_t v = (uint32_t)v64;
    const int lane = lane_id();
    const int l = a.layer;
    if (a.g.dead[v]) return;
    const int capl = a.g.layers[l].cap;
    const int d = min(a.g.layers[l].deg[v], capl);
    if (d <= 0) return;
    int32_t* row = a.g.layers[l].adj + (size_t)v * capl;
    float* rowd = a.g.layers[l].adjd + (size_t)v * capl;
    const uint32_t nb = lane < d ? guard_id(a.g, (uint32_t)row[lane]) : 0u;
    const bool nd = lane < d && a.g.dead[nb];
    const unsigned long long mdead = __ballot(nd);
    if (!mdead) return;
    const unsigned long long below = (1ull << lane) - 1ull;
    const unsigned long long mlive = __ballot(lane < d && !nd);
    if (lane < d && !nd) pid[__popcll(mlive & below)] = nb;
    int np = __popcll(mlive);
    for (unsigned long long m = mdead; m; m &= m - 1) {
        const int j = __ffsll((long long)m) - 1;
        const uint32_t x = rl_u(nb, j);
        const int dx = min(a.g.layers[l].deg[x], capl);
        if (dx <= 0) continue;
        const uint32_t y = lane < dx ? guard_id(a.g, (uint32_t)a.g.layers[l].adj[(size_t)x * capl + lane]) : 0u;
        const bool ok = lane < dx && y != v && !a.g.dead[y];
        const unsigned long long my = __ballot(ok);
        const int pos = np + __popcll(my & below);
        if (ok && pos < REPAIR_POOL) pid[pos] = y;
        np = min(np + __popcll(my), REPAIR_POOL);
    }
    __syncthreads();
    QReg<C> q;
    load_query(q, a.g.vecs + (size_t)v * a.g.pitch);
    const float qn = a.g.norms[v];
    const float inf = __int_as_float(0x7f800000);
    WaveStats st;
    for (int base = 0; base < np; base += 64) {
        const int cnt = min(64, np - base);
        const uint32_t cid = lane < cnt ? pid[base + lane] : 0u;
        int t = base;
        st.E += cnt;
        eval_list<C, G>(a.g, q, qn, cid, cnt, a.g.metric, [&](float dd, uint32_t) {
            if (lane == 0) pd[t] = dd != dd ? inf : dd;  // NaN (zero vectors) ranks last
            ++t;
        });
    }
    __syncthreads();
    for (int e = lane; e < np; e += 64) {  // rank by (dist, id); duplicates keep gather order
        const float md = pd[e];
        const uint32_t mi = pid[e];
        int rank = 0;
        for (int f = 0; f < np; ++f) {
            const float fd = pd[f];
            const uint32_t fi = pid[f];
            rank += (lt_di(fd, fi, md, mi) || (fd == md && fi == mi && f < e)) ? 1 : 0;
        }
        sdd[rank] = md;
        sid[rank] = mi;
    }
    __syncthreads();
    uint32_t kept = 0;  // lane j holds the j-th kept id
    float keptd = 0.f;
    int nkeep = 0;
    for (int i = 0; i < np && nkeep < a.mcap; ++i) {
        const uint32_t c = sid[i];
        if (i > 0 && c == sid[i - 1]) continue;
        const float dcv = sdd[i];
        bool good = true;
        if (a.heuristic && nkeep > 0) {
            QReg<C> qc;
            load_query(qc, a.g.vecs + (size_t)c * a.g.pitch);
            const float cn = a.g.norms[c];
            st.E += nkeep;
            eval_list<C, G>(a.g, qc, cn, kept, nkeep, a.g.metric, [&](float dcs, uint32_t) {
                if (dcs < dcv) good = false;
            });
        }
        if (good) {
            if (lane == nkeep) {
                kept = c;
                keptd = dcv;
            }
            ++nkeep;
        }
    }
    if (a.keep_pruned) {
        for (int i = 0; i < np && nkeep < a.mcap; ++i) {
            const uint32_t c = sid[i];
            if (i > 0 && c == sid[i - 1]) continue;
            if (__ballot(lane < nkeep && kept == c)) continue;
            if (lane == nkeep) {
                kept = c;
                keptd = sdd[i];
            }
            ++nkeep;
        }
    }
    if (lane < nkeep) {
        row[lane] = (int32_t)kept;
        rowd[lane] = keptd;
    }
    if (lane == 0) {
        a.g.layers[l].deg[v] = nkeep;
        atomicAdd(&a.stats[0], st.E);
        if (a.repaired) atomicAdd(a.repaired, 1ull);
    }
}

template <int L, int V>
int launch_batch_descend_cfg(const BatchBuildArgs& a, hipStream_t s) {
    using C = Cfg<L, V>;
    constexpr int G = cfg_group<L, V>();
    const int64_t n = a.n1 - a.n0;
    if (n <= 0) return 0;
    return a.g.h16 ? launch_grid(k_batch_descend<C, G, true>, n, 64, batch_vis_words(a), a, s)
                   : launch_grid(k_batch_descend<C, G, false>, n, 64, batch_vis_words(a), a, s);
}

// f(std::integral_constant<int, R>()) for the list of R registers that holds ef entries; -4: past the widest
template <class F>
int batch_with_list(int ef, F&& f) {
    if (ef <= 64) return f(std::integral_constant<int, 1>());
    if (ef <= 128) return f(std::integral_constant<int, 2>());
    if (ef <= 256) return f(std::integral_constant<int, 4>());
    if (ef <= 512) return f(std::integral_constant<int, 8>());
    return -4;
}

// MH_BUILD_GMAX (a build flag, default 8): cap on the rows in flight per wave
// step of the batched insert's search kernel
#ifndef MH_BUILD_GMAX
#define MH_BUILD_GMAX 8
#endif

// The kernels of one (configuration, XW): k_batch_search for R 1 / 2 / 4 / 8 with
// and without the fp16 screen (same graph, fewer bytes per candidate), and from
// XW 2 k_batch_search_mw for the narrow launches, screened only.  XW is a
// template argument: one search variant per kernel keeps it spill-free.
template <int L, int V, int XW>
int launch_batch_search_cfg(const BatchBuildArgs& a, hipStream_t s) {
    using C = Cfg<L, V>;
    constexpr int G = std::min(cfg_group<L, V>(), MH_BUILD_GMAX);
    return batch_with_list(a.ef, [&](auto regs) {
        constexpr int R = decltype(regs)::value;
        const int lds_mw = batch_vis_words(a);
        const int lds = lds_mw + (R >= 4 ? BL_MERGE_WORDS : 0);  // (the one-wave kernel's merge scratch)
        const int64_t n = a.order ? a.count : a.n1 - a.n0;
        if (n <= 0) return 0;
        if constexpr (XW >= 2) {
            if (a.g.h16 && n <= a.mw_max)  // a narrow launch: a workgroup per insert
                return launch_grid(k_batch_search_mw<C, R, G, true, XW>, n, 64 * BMW_WAVES, lds_mw, a, s);
        }
        return a.g.h16 ? launch_grid(k_batch_search<C, R, G, true, XW>, n, 64, lds, a, s)
                       : launch_grid(k_batch_search<C, R, G, false, XW>, n, 64, lds, a, s);
    });
}

template <int L, int V>
int launch_batch_commit_cfg(const BatchBuildArgs& a, int64_t max_touched, hipStream_t s) {
    constexpr int G = std::min(cfg_group<L, V>(), 4);  // rows in flight per wave step of the overflow selection
    // (the kernel strides over the touched rows: a bounded grid)
    return launch_grid(k_batch_commit<Cfg<L, V>, G>, std::min<int64_t>(max_touched, 32768), 64, 0, a, s);
}

template <int L, int V>
int launch_delete_repair_cfg(const DeleteArgs& a, hipStream_t s) {
    constexpr int G = std::min(cfg_group<L, V>(), 4);  // as k_batch_commit: the same selection
    return launch_grid(k_delete_repair<Cfg<L, V>, G>, a.n, 64, 0, a, s);
}

}  // namespace mh
