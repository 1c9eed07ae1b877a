// build_link.hpp -- the batched insert's link pass (option "batch_link"),
// instantiated per configuration in build_units.hip.  k_batch_search reads the
// graph as it stood before the batch, so a batch's rows never select each
// other.  After layer l's commit every batch row is in the layer, reachable
// through its reverse edges: k_batch_link searches the layer once more from
// the nearest row the insert search found, takes the batch-mates it meets into
// the row's neighbour selection (select_neighbours, the insert's own) and
// stages the new row; k_batch_link_apply (build.hip) copies the staged rows into the
// adjacency, and k_batch_commit merges the reverse proposals (DESIGN.md §6,
// "Linking a batch's rows").
#pragma once
#include "build_batch.hpp"

namespace mh {

template <int L, int V, int XW>
int launch_batch_link_cfg(const BatchBuildArgs& a, const LinkArgs& k, hipStream_t s);

// the one argument of the link kernels (launch_grid): the layer's insert arguments, with
// a.ef the link width, and the staging area
struct LinkKernelArgs {
    BatchBuildArgs a;
    LinkArgs k;
};

// One batch row u of layer a.layer (a.ef: the link search's width).  The
// kernel only reads the graph -- every batch row is being read by other waves
// -- and writes the staging rows and the reverse-proposal buffers.
//   C(u) = row(u) with its stored distances, and the rows of the search list
//          that are batch-mates (n0 <= c < n1, c != u, not deleted);
// old rows the search finds beyond row(u) are no candidates: the insert
// search judged them at the same width.  C(u) is ranked by (distance, id) in
// a list of the search's tier (its best 64 R entries, should it hold more)
// and selected like an insert's row.  u itself is found at distance 0 -- it is
// in the graph now -- and is left out here, so it costs the search one entry.
template <class C, int R, int G, bool SCREEN, int XW>
__global__ __launch_bounds__(64, MH_BUILD_WPS) void k_batch_link(LinkKernelArgs ka) {
    const BatchBuildArgs& a = ka.a;
    const LinkArgs& k = ka.k;
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    uint32_t u;
    if (!batch_node(a, u)) return;
    const int l = a.layer;
    if (a.levels[u] < l) return;  // (the unfused launch covers the whole batch)
    const int lane = lane_id();
    const int64_t slot = (int64_t)u - a.n0;
    WaveStats st;
    QReg<C> q;
    load_query(q, a.g.vecs + (size_t)u * a.g.pitch);
    const float qn = a.g.norms[u];
    BList<R> L;
    constexpr bool MRG = R >= 4;
    float* mrg = MRG ? reinterpret_cast<float*>(smem + batch_vis_words(a)) : nullptr;
    beam_layer<C, R, G, false, SCREEN, XW, MRG>(a.g, l, a.cur_entry[u], a.ef, q, qn, L, smem, batch_vsize(a), st,
                                                WaveBatch(), mrg);
    // row(u)
    const int capl = a.g.layers[l].cap;
    const int d0 = max(min(min(a.g.layers[l].deg[u], capl), 64), 0);
    const float inf = __int_as_float(0x7f800000);
    const uint32_t oid = lane < d0 ? guard_id(a.g, (uint32_t)a.g.layers[l].adj[(size_t)u * capl + lane]) : EMPTY_ID;
    const float od = lane < d0 ? a.g.layers[l].adjd[(size_t)u * capl + lane] : inf;
    // C(u): row(u) first, so that a batch-mate already in the row keeps its stored distance
    constexpr int NC = R * 64;
    BList<R> Cu;
    bl_init(Cu);
    for (int j = 0; j < d0; ++j) {
        const uint32_t c = rl_u(oid, j);
        if (c != u) bl_insert(Cu, NC, rl_f(od, j), c);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const uint32_t c = L.i[r] & ID_MASK;
        const bool mate = L.i[r] != EMPTY_ID && r * 64 + lane < a.ef && (int64_t)c >= a.n0 && (int64_t)c < a.n1 &&
                          c != u && !is_dead(a.g, c);
        for (unsigned long long m = __ballot(mate); m; m &= m - 1) {
            const int j = __ffsll((long long)m) - 1;
            bl_insert(Cu, NC, rl_f(L.d[r], j), rl_u(L.i[r], j) & ID_MASK);
        }
    }
    uint32_t sel = 0;
    float seld = 0.f;
    const int nsel = select_neighbours<C, R, G, SCREEN>(a, Cu, NC, sel, seld, st);
    // the neighbours new to the row: batch-mates by construction
    bool inold = false;
    for (int j = 0; j < d0; ++j) inold |= rl_u(oid, j) == sel;
    const bool fresh = lane < nsel && !inold;
    const unsigned long long mnew = __ballot(fresh);
    if (nsel == d0 && !mnew) {  // the same row: nothing staged, nothing proposed
        if (lane == 0) k.deg[slot] = -1;
    } else {
        if (lane < nsel) {
            k.adj[(size_t)slot * k.stride + lane] = (int32_t)sel;
            k.adjd[(size_t)slot * k.stride + lane] = seld;
        }
        if (fresh) {
            const int p = atomicAdd(&a.inc_cnt[sel], 1);
            if (p < a.inc_cap) {
                a.inc_src[(size_t)sel * a.inc_cap + p] = u;
                a.inc_dist[(size_t)sel * a.inc_cap + p] = seld;
            } else {
                atomicAdd(&a.stats[2], 1ull);
            }
            if (p == 0) {
                const int t = atomicAdd(a.touched_cnt, 1);
                a.touched[t] = sel;
            }
        }
        if (lane == 0) {
            k.deg[slot] = nsel;
            atomicAdd(&k.cnt[0], 1ull);
            atomicAdd(&k.cnt[1], (unsigned long long)__popcll(mnew));
        }
    }
    batch_stats(a, st);
}

// The kernels of one (configuration, XW): k_batch_link for R 1 / 2 / 4 / 8 with
// and without the fp16 screen -- k_batch_search's one-wave tiers and LDS.
template <int L, int V, int XW>
int launch_batch_link_cfg(const BatchBuildArgs& a, const LinkArgs& k, hipStream_t s) {
    using C = Cfg<L, V>;
    constexpr int G = std::min(cfg_group<L, V>(), MH_BUILD_GMAX);
    return batch_with_list(a.ef, [&](auto regs) {
        constexpr int R = decltype(regs)::value;
        const int lds = batch_vis_words(a) + (R >= 4 ? BL_MERGE_WORDS : 0);
        const int64_t n = a.order ? a.count : a.n1 - a.n0;
        if (n <= 0) return 0;
        const LinkKernelArgs p{a, k};
        return a.g.h16 ? launch_grid(k_batch_link<C, R, G, true, XW>, n, 64, lds, p, s)
                       : launch_grid(k_batch_link<C, R, G, false, XW>, n, 64, lds, p, s);
    });
}

}  // namespace mh
