// beam.hpp -- the batched beam search kernel (k_search_beam) and the
// dimension-configuration list, shared by search.hip (dispatch) and the
// beam_*.hip translation units that instantiate it per configuration (split
// so that the kernel's 4 list widths x 2 screen modes x 10 configurations
// compile in parallel).  Past the register lists (max(ef, k) > 512) the same
// search runs on a list held in LDS: k_search_beam_lds, instantiated per
// configuration, screen mode and XW in beam_w*.hip.
#pragma once
#include "device_search.hpp"
#include "engine.hpp"

namespace mh {

// group width per configuration (rows in flight per wave step)
#define MH_FOR_EACH_CFG(X)      \
    X(16, 1, 2)                 \
    X(32, 1, 4)                 \
    X(64, 1, 8)                 \
    X(64, 2, 8)                 \
    X(64, 3, 8)                 \
    X(64, 4, 4)                 \
    X(64, 6, 4)                 \
    X(64, 8, 2)            \
    X(64, 12, 1)           \
    X(64, 16, 1)

// XW: entries expanded per step of the layer-0 search (option "search_expand";
// 1 = the standard best-first search).  XW 1 is instantiated in beam_a-d.hip,
// XW 2 and 4 in beam_x2a/b.hip and beam_x4a/b.hip.
template <int L, int V, int XW>
int launch_beam_cfg(const SearchArgs& a, hipStream_t s);

// ---------------------------------------------------------------------------
// batched search: one wave per query
// ---------------------------------------------------------------------------
// One query b: greedy descent, the layer-0 beam, and its first k live entries
// into the outputs.  BEv scores each batch of candidates (beam_layer).
// the visited set's LDS words (the merge scratch follows it)
__host__ __device__ inline int beam_vis_words(const SearchArgs& a) { return a.vis16 ? VIS16_WORDS : a.vis_n; }

// The ordered path splits the descent: the pre-pass walks the layers of the sort
// key and above, top .. beam_order_lo, and the layer-0 launch walks the rest
// from where it stopped (the walks of the upper layers are what the queries of
// a cell share; splitting below the key keeps the pre-pass short).
__host__ __device__ inline int beam_order_lo(const SearchArgs& a) { return a.key_n > 0 ? a.key_top - a.key_n + 1 : 1; }

// the greedy descent (ef = upper_ef) from node ep through the layers l_hi .. l_lo
// (the whole descent: the top layer's entry, top .. 1); to0: down to layer 0's
// entry.  KEY (the ordered path's pre-pass): *key collects the node the descent
// stood on when it left each of the layers key_top .. key_top - key_n + 1, the
// highest layer in the most significant bits.
template <class C, int G, bool SCREEN, bool KEY = false, class BEv>
__device__ __forceinline__ uint32_t beam_descend(const SearchArgs& a, const QReg<C>& q, float qn, uint32_t* smem,
                                                 int vsz, WaveStats& st, const BEv& bev, uint32_t ep, int l_hi,
                                                 int l_lo, bool to0, unsigned long long* key = nullptr) {
    {
        BList<1> L1;
        for (int l = l_hi; l >= l_lo; --l) {  // greedy descent, ef = 1
            bool skip = false;
            if (a.g.layers[l].deg[ep] == -2) {  // not in this layer: restart at its entry
                const int32_t e = a.layer_entry[l];
                if (e < 0)
                    skip = true;
                else
                    ep = (uint32_t)e;
            }
            if (!skip) {
                beam_layer<C, 1, G, false, SCREEN, 1>(a.g, l, ep, a.upper_ef, q, qn, L1, smem, vsz, st, bev);
                float d;
                uint32_t id;
                bl_at(L1, 0, d, id);
                if (id != EMPTY_ID) ep = id & ID_MASK;
            }
            if constexpr (KEY) {  // (every query shifts the same number of fields in)
                if (l <= a.key_top && l > a.key_top - a.key_n) {
                    // a field narrower than an id holds a hash of it: two cells that collide are
                    // merely sorted together
                    const uint32_t f = a.key_hash ? (ep * 2654435761u) >> (32 - a.key_id_bits)
                                                  : ep & ((1u << a.key_id_bits) - 1u);
                    *key = (*key << a.key_id_bits) | (unsigned long long)f;
                }
            }
        }
    }
    if (to0 && a.g.layers[0].deg[ep] == -2) ep = (uint32_t)a.layer_entry[0];
    return ep;
}

// where query b's descent in the layer-0 kernels starts: the top layer's entry,
// or (ordered path) the node and the layer the pre-pass stopped above
__device__ __forceinline__ uint32_t beam_entry_of(const SearchArgs& a, int64_t b) {
    return a.order ? uni(a.ep0[b]) : a.entry;
}
__device__ __forceinline__ int beam_entry_layer(const SearchArgs& a) { return a.order ? beam_order_lo(a) - 1 : a.top; }

// rows [nvalid, k) of query b's outputs: no result
__device__ __forceinline__ void beam_pad_out(const SearchArgs& a, int64_t b, int nvalid) {
    const int lane = lane_id();
    for (int i = nvalid + lane; i < a.k; i += 64) {
        a.out_keys[b * a.k + i] = (int64_t)-1;
        a.out_dist[b * a.k + i] = __int_as_float(0x7f800000);
        if (a.out_ids) a.out_ids[b * a.k + i] = -1;
    }
    if (lane == 0) a.out_n[b] = nvalid;
}

template <class C, int R, int G, bool SCREEN, int XW, class BEv>
__device__ __forceinline__ void beam_query(const SearchArgs& a, int64_t b, const QReg<C>& q, float qn, uint32_t* smem,
                                           WaveStats& st, const BEv& bev) {
    const int lane = lane_id();
    const int vsz = a.vis16 ? -1 : a.vis_n;  // (beam_layer: < 0 selects the compact set)
    const uint32_t ep = beam_descend<C, G, SCREEN>(a, q, qn, smem, vsz, st, bev, beam_entry_of(a, b),
                                                   beam_entry_layer(a), 1, true);
    BList<R> L;
    const int efl = a.ef > a.k ? a.ef : a.k;
    // lists of 256 / 512 entries merge each step's candidates at once, with the
    // LDS past the visited set as scratch (launch_beam_t sizes the LDS for it;
    // the default compact set leaves room in the 20 KiB a 2-wave SIMD allows)
    constexpr bool MRG = R >= 4;
    float* mrg = MRG ? reinterpret_cast<float*>(smem + beam_vis_words(a)) : nullptr;
    beam_layer<C, R, G, false, SCREEN, XW, MRG>(a.g, 0, ep, efl, q, qn, L, smem, vsz, st, bev, mrg);
    // compact the sorted list into the first k live entries (deleted rows
    // route the search but are never returned)
    int nvalid = 0;
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const uint32_t id = L.i[r] & ID_MASK;
        const bool ok = L.i[r] != EMPTY_ID && !is_dead(a.g, id);
        const unsigned long long m = __ballot(ok);
        const int pos = nvalid + __popcll(m & below);
        if (ok && pos < a.k) {
            a.out_keys[b * a.k + pos] = a.g.keys[id];
            a.out_dist[b * a.k + pos] = L.d[r];
            if (a.out_ids) a.out_ids[b * a.k + pos] = (int32_t)id;
        }
        nvalid += __popcll(m);
    }
    beam_pad_out(a, b, min(nvalid, a.k));
}

// The query of workgroup i.  Fused path: query i.  Ordered path: the query at
// sorted position i, or with order_chunk at position (i % 8) * chunk + i / 8:
// workgroups i and i + 8 have been observed to share an XCD, so each XCD then
// walks one contiguous run of the sorted queries (speed only: any mapping that
// covers every position once is correct).  -1: nothing to do.
__device__ __forceinline__ int64_t beam_query_of(const SearchArgs& a, int64_t i) {
    if (!a.order) return i < a.B ? i : -1;
    const int64_t pos = a.order_chunk > 0 ? (i & 7) * a.order_chunk + (i >> 3) : i;
    if (pos >= a.B || (a.order_chunk > 0 && (i >> 3) >= a.order_chunk)) return -1;
    const uint32_t b = uni(a.order[pos]);
    return b < (uint64_t)a.B ? (int64_t)b : -1;
}

__device__ __forceinline__ void beam_stats(const SearchArgs& a, const WaveStats& st) {
    if (lane_id() == 0) {
        atomicAdd(&a.stats[0], st.E);
        atomicAdd(&a.stats[1], st.X);
        if (st.resets) atomicAdd(&a.stats[2], st.resets);
        atomicAdd(&a.stats[8], st.S);
        atomicAdd(&a.stats[9], st.F);
#ifdef MH_PROF_BEAM
        // (tools-only: the slots the batched insert uses, read back as build_screened /
        // build_f32_rows / exact_uncertified)
        atomicAdd(&a.stats[10], st.c_ins);
        atomicAdd(&a.stats[11], st.c_score);
        atomicAdd(&a.stats[3], st.c_all);
#endif
    }
}

// MH_BEAM_WIDE_G / MH_BEAM_WIDE_WAVES (build flags, for tools/ variants): rows
// in flight per wave step and the waves per SIMD the compiler must fit, for the
// 512-entry list (R = 8); 0 = the configuration's G and 2 waves
#ifndef MH_BEAM_WIDE_G
#define MH_BEAM_WIDE_G 0
#endif
#ifndef MH_BEAM_WIDE_WAVES
#define MH_BEAM_WIDE_WAVES 2
#endif
template <class C, int R, int G, bool SCREEN, int XW>
__global__ __attribute__((amdgpu_flat_work_group_size(64, 64), amdgpu_waves_per_eu(R >= 8 ? MH_BEAM_WIDE_WAVES : 2)))
void k_search_beam(SearchArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    const int64_t b = beam_query_of(a, blockIdx.x);
    if (b < 0) return;
    QReg<C> q;
    load_query(q, a.q + (size_t)b * C::PITCH);
    const float qn = query_norm(q);
    WaveStats st;
    beam_query<C, R, G, SCREEN, XW>(a, b, q, qn, smem, st, WaveBatch());
    beam_stats(a, st);
}

// ---------------------------------------------------------------------------
// small batches (the reference's ParallelSearch, graph.go:631-790: one query's
// neighbour distances fanned out over workers): one workgroup of BMW_WAVES
// waves per query.  Wave 0 runs the list, the visited set and the expansions
// exactly as k_search_beam; each batch of new candidates is split over the
// waves (screen + f32 on each wave's rows, in one round trip instead of one
// per 16 rows), and the survivors come back to wave 0's list.  The list is the
// best ef of everything inserted whatever the insertion order, so the results
// are k_search_beam's bit for bit (test_gpu_parity.py: batches below and above
// BMW_MAX_B compared).
// ---------------------------------------------------------------------------
// (BmwShare, MwBatch: device_search.hpp, shared with the batched insert)
template <class C, int R, int G, bool SCREEN>
__global__ __launch_bounds__(64 * BMW_WAVES) void k_search_beam_mw(SearchArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    __shared__ BmwShare sh;
    const int64_t b = blockIdx.x;
    if (b >= a.B) return;  // (whole workgroup)
    const int wave = threadIdx.x >> 6;
    QReg<C> q;
    load_query(q, a.q + (size_t)b * C::PITCH);
    const float qn = query_norm(q);
    WaveStats st;
    if (wave == 0) {
        beam_query<C, R, G, SCREEN, 1>(a, b, q, qn, smem, st, MwBatch{&sh});
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
    beam_stats(a, st);
}

// ---------------------------------------------------------------------------
// ordered path, pre-pass: the descent through the layers top .. beam_order_lo
// alone, one wave per query, with the fused kernels' upper_ef, visited set and
// screen.  Writes the node it stopped on, the sort key of the descent path and
// the sort's value (the query's index); its counters go into the same slots as
// the layer-0 launch's, which walks the remaining layers.
// ---------------------------------------------------------------------------
template <class C, int G, bool SCREEN>
__global__ __attribute__((amdgpu_flat_work_group_size(64, 64))) void k_beam_descend(SearchArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    const int64_t b = blockIdx.x;
    if (b >= a.B) return;
    QReg<C> q;
    load_query(q, a.q + (size_t)b * C::PITCH);
    const float qn = query_norm(q);
    WaveStats st;
    const int vsz = a.vis16 ? -1 : a.vis_n;
    unsigned long long key = 0;
    const uint32_t ep =
        beam_descend<C, G, SCREEN, true>(a, q, qn, smem, vsz, st, WaveBatch(), a.entry, a.top, beam_order_lo(a), false, &key);
    if (lane_id() == 0) {
        a.ep0[b] = ep;
        a.okey[b] = key;
        a.oidx[b] = (uint32_t)b;
    }
    beam_stats(a, st);
}

template <class C, int R, int G, int XW>
static int launch_beam_t(const SearchArgs& a, hipStream_t s) {
    const size_t lds = (size_t)4 * (size_t)(R >= 4 ? std::max(a.vis_n, beam_vis_words(a) + BL_MERGE_WORDS) : a.vis_n);
    // small batch: a workgroup per query (the standard search only; a wider
    // expansion runs the one-wave kernel at every batch size)
    if constexpr (XW == 1) {
        if (R <= 2 && beam_small_batch(a) && !a.order) {
            if (a.g.h16)
                hipLaunchKernelGGL((k_search_beam_mw<C, R, G, true>), dim3((unsigned)a.B), dim3(64 * BMW_WAVES), lds, s,
                                   a);
            else
                hipLaunchKernelGGL((k_search_beam_mw<C, R, G, false>), dim3((unsigned)a.B), dim3(64 * BMW_WAVES), lds,
                                   s, a);
            return hipGetLastError() == hipSuccess ? 0 : -1;
        }
    }
    const unsigned grid = (unsigned)(a.order ? beam_order_grid(a) : a.B);
    if (a.g.h16)
        hipLaunchKernelGGL((k_search_beam<C, R, G, true, XW>), dim3(grid), dim3(64), lds, s, a);
    else
        hipLaunchKernelGGL((k_search_beam<C, R, G, false, XW>), dim3(grid), dim3(64), lds, s, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---------------------------------------------------------------------------
// wide lists (beam_lds_min_ef <= max(ef, k) <= LL_MAX_EF): the layer-0 list in
// LDS (device_search.hpp LList) behind the visited set; one wave per query at
// every batch size and every XW.  The descent, the step structure, the screen
// and the visited set are k_search_beam's (beam_layer_l over the other list),
// so the results are the register lists' at equal ef.
// ---------------------------------------------------------------------------
template <class C, int G, bool SCREEN, int XW>
__global__ __attribute__((amdgpu_flat_work_group_size(64, 64))) void k_search_beam_lds(SearchArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    const int64_t b = beam_query_of(a, blockIdx.x);
    if (b < 0) return;
    const int lane = lane_id();
    QReg<C> q;
    load_query(q, a.q + (size_t)b * C::PITCH);
    const float qn = query_norm(q);
    WaveStats st;
    const WaveBatch bev;
    const int vsz = a.vis16 ? -1 : a.vis_n;
    const uint32_t ep = beam_descend<C, G, SCREEN>(a, q, qn, smem, vsz, st, bev, beam_entry_of(a, b),
                                                   beam_entry_layer(a), 1, true);
    const int efl = a.ef > a.k ? a.ef : a.k;
    LList L;
    ll_place(L, smem + ((beam_vis_words(a) + 3) & ~3), efl);
    beam_layer_l<C, LList, G, false, SCREEN, XW, true, WaveBatch>(a.g, 0, ep, efl, q, qn, L, smem, vsz, st, bev, nullptr);
    // the first k live entries (deleted rows route the search but are never returned)
    int nvalid = 0;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int c = 0; c < L.n && nvalid < a.k; c += 64) {
        const int idx = c + lane;
        const uint32_t w = idx < L.n ? L.i[idx] : EMPTY_ID;
        const uint32_t id = w & ID_MASK;
        const bool ok = w != EMPTY_ID && !is_dead(a.g, id);
        const unsigned long long m = __ballot(ok);
        const int pos = nvalid + __popcll(m & below);
        if (ok && pos < a.k) {
            a.out_keys[b * a.k + pos] = a.g.keys[id];
            a.out_dist[b * a.k + pos] = L.d[idx];
            if (a.out_ids) a.out_ids[b * a.k + pos] = (int32_t)id;
        }
        nvalid += __popcll(m);
    }
    beam_pad_out(a, b, min(nvalid, a.k));
    beam_stats(a, st);
}

// the wide tier's dynamic LDS: the visited set, then the list
inline size_t beam_lds_bytes(const SearchArgs& a) {
    const int efl = a.ef > a.k ? a.ef : a.k;
    return (size_t)4 * (size_t)(((beam_vis_words(a) + 3) & ~3) + ll_words(efl));
}
constexpr size_t BEAM_LDS_MAX_BYTES = 64 * 1024;  // a workgroup's LDS without an opt-in attribute

// -2: the visited set and the list do not fit a workgroup's LDS (an explicit
// vis_entries too large for this ef); -4: past the list's capacity
template <class C, int G, int XW>
static int launch_beam_lds_t(const SearchArgs& a, hipStream_t s) {
    const int efl = a.ef > a.k ? a.ef : a.k;
    if (efl > LL_MAX_EF) return -4;
    const size_t lds = beam_lds_bytes(a);
    if (lds > BEAM_LDS_MAX_BYTES) return -2;
    const unsigned grid = (unsigned)(a.order ? beam_order_grid(a) : a.B);
    if (a.g.h16)
        hipLaunchKernelGGL((k_search_beam_lds<C, G, true, XW>), dim3(grid), dim3(64), lds, s, a);
    else
        hipLaunchKernelGGL((k_search_beam_lds<C, G, false, XW>), dim3(grid), dim3(64), lds, s, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// group width G of configuration (L, V), from MH_FOR_EACH_CFG
template <int L, int V>
constexpr int beam_group() {
#define X_(L_, V_, G_) \
    if (L == L_ && V == V_) return G_;
    MH_FOR_EACH_CFG(X_)
#undef X_
    return 0;
}

template <int L, int V, int XW>
int launch_beam_cfg(const SearchArgs& a, hipStream_t s) {
    constexpr int G = beam_group<L, V>();
    const int efl = a.ef > a.k ? a.ef : a.k;
    if (efl <= 64) return launch_beam_t<Cfg<L, V>, 1, G, XW>(a, s);
    if (efl <= 128) return launch_beam_t<Cfg<L, V>, 2, G, XW>(a, s);
    if (efl <= 256) return launch_beam_t<Cfg<L, V>, 4, G, XW>(a, s);
    constexpr int GW = MH_BEAM_WIDE_G > 0 && MH_BEAM_WIDE_G < G ? MH_BEAM_WIDE_G : G;
    if (efl <= 512) return launch_beam_t<Cfg<L, V>, 8, GW, XW>(a, s);
    return -4;
}

// instantiated per XW in beam_wa-wc.hip
template <int L, int V, int XW>
int launch_beam_lds_cfg(const SearchArgs& a, hipStream_t s) {
    return launch_beam_lds_t<Cfg<L, V>, beam_group<L, V>(), XW>(a, s);
}

// the ordered path's pre-pass (k_beam_descend), instantiated in beam_desc.hip.
// The same failures as the layer-0 launch it precedes: -4 past the LDS list's
// capacity, -2 when the visited set and the list do not fit a workgroup's LDS.
template <int L, int V>
int launch_beam_descend_cfg(const SearchArgs& a, hipStream_t s) {
    using C = Cfg<L, V>;
    constexpr int G = beam_group<L, V>();
    const int efl = a.ef > a.k ? a.ef : a.k;
    if (efl >= a.lds_min_ef) {
        if (efl > LL_MAX_EF) return -4;
        if (beam_lds_bytes(a) > BEAM_LDS_MAX_BYTES) return -2;
    } else if (efl > 512) {
        return -4;
    }
    const size_t lds = (size_t)4 * (size_t)std::max(a.vis_n, beam_vis_words(a));
    if (a.g.h16)
        hipLaunchKernelGGL((k_beam_descend<C, G, true>), dim3((unsigned)a.B), dim3(64), lds, s, a);
    else
        hipLaunchKernelGGL((k_beam_descend<C, G, false>), dim3((unsigned)a.B), dim3(64), lds, s, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace mh
