// beam.hpp -- the batched beam search kernels and their launchers, shared by
// search.hip (dispatch) and beam_units.hip, which instantiates them per
// configuration in its units (split so that the 4 list widths x 2 screen
// modes x 10 configurations compile in parallel).  One body, beam_query, runs
// a query over either list: BList<R> in registers (k_search_beam,
// k_search_beam_mw), or past them (max(ef, k) > 512) LList in LDS
// (k_search_beam_lds).  The filtered search (k_search_beam_filt) is the same
// body with the RowFilter policy over the LDS list.
#pragma once
#include <type_traits>

#include "device_search.hpp"
#include "engine.hpp"

namespace mh {

// XW: entries expanded per step of the layer-0 search (option "search_expand";
// 1 = the standard best-first search).  The register lists' and the LDS list's
// launchers are separate templates, so that beam_units.hip can instantiate the
// two tiers in different objects.
template <int L, int V, int XW>
int launch_beam_cfg(const SearchArgs& a, hipStream_t s);
template <int L, int V, int XW>
int launch_beam_lds_cfg(const SearchArgs& a, hipStream_t s);
template <int L, int V>
int launch_beam_filt_cfg(const SearchArgs& a, const FilterArgs& f, hipStream_t s);

// ---------------------------------------------------------------------------
// batched search: one wave per query
// ---------------------------------------------------------------------------
// the width of the layer-0 list
__host__ __device__ inline int beam_efl(const SearchArgs& a) { return a.ef > a.k ? a.ef : a.k; }
// the tier: the LDS-resident list from max(ef, k) = lds_min_ef (513 unless the
// option beam_lds_min_ef lowers it: past the widest register list)
inline bool beam_in_lds(const SearchArgs& a) { return beam_efl(a) >= a.lds_min_ef; }

// the visited set's LDS words (the list's part follows it)
__host__ __device__ inline int beam_vis_words(const SearchArgs& a) { return a.vis16 ? VIS16_WORDS : a.vis_n; }

// The dynamic LDS of a layer-0 launch over list LT, in 32-bit words: the
// kernel places the list's part at `list` (bl_place), the launcher asks for
// `words`.  Registers: bl_merge's scratch where the steps merge, and never
// less than the vis_n words of the 32-bit set, which the compact set leaves
// partly unused (the default compact set with the scratch fits the 20 KiB a
// 2-wave SIMD allows).  The host sets vis16 only with vis_n >= VIS16_WORDS
// (search_host.cpp), so for the lists that do not merge, and for a pre-pass
// that keeps the launch's set (beam_desc_vis), this is vis_n itself.  LDS: the
// list, 16-byte aligned.
struct BeamLds {
    int list, words;
};
template <class LT>
__host__ __device__ inline BeamLds beam_lds(const SearchArgs& a) {
    const int vis = beam_vis_words(a);
    if constexpr (bl_regs<LT> == 0) {
        const int at = (vis + 3) & ~3;
        return {at, at + ll_words(beam_efl(a))};
    } else {
        const int w = vis + (bl_merges<LT> ? BL_MERGE_WORDS : 0);
        return {vis, a.vis_n > w ? a.vis_n : w};
    }
}
constexpr size_t BEAM_LDS_MAX_BYTES = 64 * 1024;  // a workgroup's LDS without an opt-in attribute

// 0, or why no layer-0 launch of the given tier (lds: the LDS list, else the
// register lists) runs these arguments: -4 past the capacity of the tier's
// list, -2 when the visited set and the LDS list do not fit a workgroup's LDS
// (an explicit vis_entries too large for this ef).  Asked by both tiers'
// launches and, for the tier it precedes, by the pre-pass.
inline int beam_limits(const SearchArgs& a, bool lds) {
    if (!lds) return beam_efl(a) > 512 ? -4 : 0;
    if (beam_efl(a) > LL_MAX_EF) return -4;
    return (size_t)4 * (size_t)beam_lds<LList>(a).words > BEAM_LDS_MAX_BYTES ? -2 : 0;
}

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

// How the one body reaches the launch's arguments: through a reference in the
// register kernels and as a copy in the LDS kernel, as each did while it had a
// body of its own.  The choice only steers the compiler's schedule: with these
// two the kernels come out as they did before the bodies were shared (the
// register kernels instruction for instruction, the LDS kernel but for three
// reordered instructions), and through a reference about a fifth of the LDS
// kernel's instructions move (profiles/beam_refactor.txt, section 4).
template <class LT>
using BeamArgs = std::conditional_t<bl_regs<LT> == 0, const SearchArgs, const SearchArgs&>;

// The filtered query (k_search_beam_filt): beam_query's descent, the layer-0 body
// with the RowFilter policy, and the first k entries of its list R, which holds
// allowed live rows only.  The plain beam_query below stays a function of its own,
// word for word what it was: written as one template over the policy (or with a
// forwarding overload, which copies `a` once more for the LDS list), it changed
// the schedule of every LDS kernel and of the register kernels at 2 / 4 entries
// per step (profiles/filtered_search_build.txt); the layer-0 body is shared.
template <class C, class LT, int G, bool SCREEN, int XW, class BEv, class Flt>
__device__ __forceinline__ void beam_query_f(BeamArgs<LT> a, int64_t b, const QReg<C>& q, float qn, uint32_t* smem,
                                             WaveStats& st, const BEv& bev, Flt& flt) {
    static_assert(Flt::on, "the plain search is beam_query");
    const int lane = lane_id();
    const int vsz = a.vis16 ? -1 : a.vis_n;  // (beam_layer: < 0 selects the compact set)
    const uint32_t ep = beam_descend<C, G, SCREEN>(a, q, qn, smem, vsz, st, bev, beam_entry_of(a, b),
                                                   beam_entry_layer(a), 1, true);
    LT L;
    const int efl = beam_efl(a);
    float* mrg = bl_place(L, smem + beam_lds<LT>(a).list, efl);
    beam_layer_l<C, LT, G, false, SCREEN, XW, bl_merges<LT>, BEv>(a.g, 0, ep, efl, q, qn, L, smem, vsz, st, bev, mrg, flt);
    int nvalid = 0;
#pragma unroll
    for (int c = 0; c < bl_span(flt.R); c += 64) {
        const uint32_t id = bl_chunk_id(flt.R, c);
        const int pos = c + lane;  // (R is sorted and dense from entry 0)
        const bool ok = id != EMPTY_ID;
        if (ok && pos < a.k) {
            a.out_keys[b * a.k + pos] = a.g.keys[id];
            a.out_dist[b * a.k + pos] = bl_chunk_dist(flt.R, c);
            if (a.out_ids) a.out_ids[b * a.k + pos] = (int32_t)id;
        }
        nvalid += __popcll(__ballot(ok));
    }
    beam_pad_out(a, b, min(nvalid, a.k));
}

// One query b over list LT: the greedy descent, the layer-0 beam, and its
// first k live entries into the outputs.  BEv scores each batch of candidates
// (beam_layer_l).
template <class C, class LT, int G, bool SCREEN, int XW, class BEv>
__device__ __forceinline__ void beam_query(BeamArgs<LT> a, int64_t b, const QReg<C>& q, float qn, uint32_t* smem,
                                           WaveStats& st, const BEv& bev) {
    const int lane = lane_id();
    const int vsz = a.vis16 ? -1 : a.vis_n;  // (beam_layer: < 0 selects the compact set)
    const uint32_t ep = beam_descend<C, G, SCREEN>(a, q, qn, smem, vsz, st, bev, beam_entry_of(a, b),
                                                   beam_entry_layer(a), 1, true);
    LT L;
    NoFilter nf;
    const int efl = beam_efl(a);
    float* mrg = bl_place(L, smem + beam_lds<LT>(a).list, efl);
    beam_layer_l<C, LT, G, false, SCREEN, XW, bl_merges<LT>, BEv>(a.g, 0, ep, efl, q, qn, L, smem, vsz, st, bev, mrg, nf);
    // compact the sorted list into the first k live entries (deleted rows
    // route the search but are never returned)
    int nvalid = 0;
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (int c = 0; c < bl_span(L); c += 64) {
        if (bl_regs<LT> == 0 && nvalid >= a.k) break;  // (the LDS list stops early; the registers are all read)
        const uint32_t w = bl_chunk_id(L, c);
        const uint32_t id = w & ID_MASK;
        const bool ok = w != EMPTY_ID && !is_dead(a.g, id);
        const unsigned long long m = __ballot(ok);
        const int pos = nvalid + __popcll(m & below);
        if (ok && pos < a.k) {
            a.out_keys[b * a.k + pos] = a.g.keys[id];
            a.out_dist[b * a.k + pos] = bl_chunk_dist(L, c);
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

// one wave's whole query: load it, run it (beam_query), add the counters
template <class C, class LT, int G, bool SCREEN, int XW>
__device__ __forceinline__ void beam_wave(BeamArgs<LT> a, int64_t b, uint32_t* smem) {
    QReg<C> q;
    load_query(q, a.q + (size_t)b * C::PITCH);
    const float qn = query_norm(q);
    WaveStats st;
    beam_query<C, LT, G, SCREEN, XW>(a, b, q, qn, smem, st, WaveBatch());
    beam_stats(a, st);
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
// (the kernels keep their own attributes: the register kernel's waves per SIMD
// are its register budget, and the recorded profiles go by these names)
template <class C, int R, int G, bool SCREEN, int XW>
__global__ __attribute__((amdgpu_flat_work_group_size(64, 64), amdgpu_waves_per_eu(R >= 8 ? MH_BEAM_WIDE_WAVES : 2)))
void k_search_beam(SearchArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    const int64_t b = beam_query_of(a, blockIdx.x);
    if (b < 0) return;
    beam_wave<C, BList<R>, G, SCREEN, XW>(a, b, smem);
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
        beam_query<C, BList<R>, G, SCREEN, 1>(a, b, q, qn, smem, st, MwBatch{&sh});
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
// alone, one wave per query, with the fused kernels' upper_ef and screen.
// Writes the node it stopped on, the sort key of the descent path and the
// sort's value (the query's index).
//
// A descent is a chain of dependent round trips -- per layer the deg check and
// the entry's row, per expansion the adjacency row, the fp16 screen and the f32
// survivors -- and nothing hides it but other waves.  So the pre-pass is shaped
// for waves in flight, not for rows in flight (DESIGN.md "Query order", the
// pre-pass; measured at the headline's Cfg<64, 3>):
//  - rows in flight and registers: beam_desc_group / beam_desc_waves below, not
//    the layer-0 search's cfg_group.  Every distance is the same sum whatever G
//    (eval_rows: the lane's partial sum, then reduce_rows' one butterfly).
//  - the visited set: beam_desc_vis entries, passed as `pvis` (the size the
//    launch asked LDS for), not the layer-0 search's a.vis_n / a.vis16.
//  - the counters: E, X, S and F go to a.pstat, one store per query, and
//    k_beam_descend_stats (search.hip) adds them up into the slots the layer-0
//    launch uses; 65,536 waves' atomicAdd on the same words within a millisecond
//    queue on them (0.7 ms of the step at the headline).  A visited reset, which
//    a pre-pass hardly ever sees, is still counted where it happens.
// ---------------------------------------------------------------------------
// MH_DESC_G / MH_DESC_WAVES / MH_DESC_VIS (build flags, for tools/ variants):
// another G, waves per SIMD or visited-set size for every configuration's pre-pass
// (0 = the rule)
#ifndef MH_DESC_G
#define MH_DESC_G 0
#endif
#ifndef MH_DESC_WAVES
#define MH_DESC_WAVES 0
#endif
#ifndef MH_DESC_VIS
#define MH_DESC_VIS 0
#endif
// Rows in flight per wave step, and the waves per SIMD the compiler must fit.
// At the headline, screened: G 8 takes 213 VGPRs (2 waves), G 4 139 (3), G 2
// 105 (4), G 1 89 (5); 4 waves of G 2 and 5 of G 1 run the pre-pass equally fast
// (a narrower G takes more round trips per expansion), both ahead of G 4, and a
// target that makes the compiler spill (G 4 at 4 waves, G 2 at 6 or 8) is slower
// than the same G without it.  The rule for every configuration: G at most 2, and
// the 4 waves where the screened kernel fits their 128 registers without scratch
// (rows of up to 4 float4 per lane), else the 2 of the layer-0 kernels.
template <int L, int V>
constexpr int beam_desc_group() {
    constexpr int G = cfg_group<L, V>();
    return MH_DESC_G > 0 ? (MH_DESC_G < G ? MH_DESC_G : G) : G < 2 ? G : 2;
}
template <int L, int V>
constexpr int beam_desc_waves() {
    return MH_DESC_WAVES > 0 ? MH_DESC_WAVES : V <= 4 ? 4 : 2;
}
// The visited set: a greedy walk (upper_ef 1) probes a few tens of ids per layer
// and a walk with a list of 4 a few hundred at most, and the set is cleared at
// every layer, so up to upper_ef 4 the pre-pass takes 1,024 entries (4 KiB)
// instead of the layer-0 search's 5,120 (20 KiB, which alone held the pre-pass
// to 2 waves per SIMD).  It resets at 768 ids in ONE layer, that is after 48
// expansions of 16 neighbours there: the headline's pre-pass expands 11 nodes
// and evaluates 114 rows per query over ALL its layers (and the tests compare
// the counters with the fused launch's, resets included).  A pathological
// single-layer walk past it adds a
// reset the fused launch does not have, which changes the counters and never
// the lists.  A wider
// upper_ef, or a set the user made no larger than this, keeps the launch's own
// set.  0: the launch's own.
constexpr int BEAM_DESC_VIS = 1024, BEAM_DESC_VIS_MAX_EF = 4;
inline int beam_desc_vis(const SearchArgs& a) {
    const int n = MH_DESC_VIS > 0 ? MH_DESC_VIS : BEAM_DESC_VIS;
    return a.upper_ef <= BEAM_DESC_VIS_MAX_EF && beam_vis_words(a) > n ? n : 0;
}

template <class C, int G, bool SCREEN, int W>
__global__ __attribute__((amdgpu_flat_work_group_size(64, 64), amdgpu_waves_per_eu(W))) void k_beam_descend(SearchArgs a,
                                                                                                            int pvis) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    const int64_t b = blockIdx.x;
    if (b >= a.B) return;
    QReg<C> q;
    load_query(q, a.q + (size_t)b * C::PITCH);
    const float qn = query_norm(q);
    WaveStats st;
    const int vsz = pvis > 0 ? pvis : a.vis16 ? -1 : a.vis_n;
    unsigned long long key = 0;
    const uint32_t ep =
        beam_descend<C, G, SCREEN, true>(a, q, qn, smem, vsz, st, WaveBatch(), a.entry, a.top, beam_order_lo(a), false, &key);
    if (lane_id() == 0) {
        a.ep0[b] = ep;
        a.okey[b] = key;
        a.oidx[b] = (uint32_t)b;
        // (a descent's counts are far below 2^32)
        reinterpret_cast<uint4*>(a.pstat)[b] = make_uint4((uint32_t)st.E, (uint32_t)st.X, (uint32_t)st.S, (uint32_t)st.F);
        if (st.resets) atomicAdd(&a.stats[2], st.resets);
    }
}

// ---------------------------------------------------------------------------
// wide lists (beam_lds_min_ef <= max(ef, k) <= LL_MAX_EF): the layer-0 list in
// LDS (device_search.hpp LList) behind the visited set; one wave per query at
// every batch size and every XW.  The same body over the other list, so the
// results are the register lists' at equal ef.
// ---------------------------------------------------------------------------
template <class C, int G, bool SCREEN, int XW>
__global__ __attribute__((amdgpu_flat_work_group_size(64, 64))) void k_search_beam_lds(SearchArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    const int64_t b = beam_query_of(a, blockIdx.x);
    if (b < 0) return;
    beam_wave<C, LList, G, SCREEN, XW>(a, b, smem);
}

// ---------------------------------------------------------------------------
// filtered search (max(ef, k) <= 128, route width max(ef, k) <= a.ef <= LL_MAX_EF;
// DESIGN.md "Filtered search"): k_search_beam_lds's wave with the RowFilter
// policy.  a.ef is the ROUTE width (the LDS list's), f.ef the result width; the
// fused launch only, one entry expanded per step.
// ---------------------------------------------------------------------------
template <class C, int G, bool SCREEN>
__global__ __attribute__((amdgpu_flat_work_group_size(64, 64))) void k_search_beam_filt(SearchArgs a, FilterArgs f) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    const int64_t b = blockIdx.x;
    if (b >= a.B) return;
    RowFilter flt;
    flt.E = f.ef;
    flt.bits = nullptr;
    const int32_t fi = uni(f.filter_of[b]);
    if (fi != -1) {  // (-1: every live row)
        const uint32_t* bits = fi >= 0 && fi < f.nslots ? f.filters[fi] : nullptr;
        if (!bits) {  // names no filter: no results, reported like the other device errors
            if (lane_id() == 0) atomicOr(a.err, 8);
            beam_pad_out(a, b, 0);
            return;
        }
        flt.bits = bits;
    }
    QReg<C> q;
    load_query(q, a.q + (size_t)b * C::PITCH);
    const float qn = query_norm(q);
    WaveStats st;
    beam_query_f<C, LList, G, SCREEN, 1>(a, b, q, qn, smem, st, WaveBatch(), flt);
    beam_stats(a, st);
}

// f(std::true_type / std::false_type): the kernels with and without the fp16 screen
template <class F>
int beam_with_screen(const SearchArgs& a, F&& f) {
    return a.g.h16 ? f(std::true_type()) : f(std::false_type());
}

// the layer-0 launch over list LT
template <class C, class LT, int G, int XW>
static int launch_beam_t(const SearchArgs& a, hipStream_t s) {
    static_assert(bl_regs<LT> >= 0, "BList<R> or LList");
    const int lds = beam_lds<LT>(a).words;
    return beam_with_screen(a, [&](auto screen) {
        constexpr bool SC = decltype(screen)::value;
        constexpr int R = bl_regs<LT>;
        // small batch: a workgroup per query (the standard search on the narrow
        // register lists only; a wider expansion and the LDS list run the one-wave
        // kernel at every batch size)
        if constexpr (XW == 1 && R >= 1) {
            if (R <= 2 && beam_small_batch(a) && !a.order)
                return launch_grid(k_search_beam_mw<C, R, G, SC>, a.B, 64 * BMW_WAVES, lds, a, s);
        }
        const int64_t grid = a.order ? beam_order_grid(a) : a.B;
        if constexpr (R == 0)
            return launch_grid(k_search_beam_lds<C, G, SC, XW>, grid, 64, lds, a, s);
        else
            return launch_grid(k_search_beam<C, R, G, SC, XW>, grid, 64, lds, a, s);
    });
}

template <int L, int V, int XW>
int launch_beam_cfg(const SearchArgs& a, hipStream_t s) {
    using C = Cfg<L, V>;
    constexpr int G = cfg_group<L, V>();
    if (const int rc = beam_limits(a, false)) return rc;
    const int efl = beam_efl(a);
    if (efl <= 64) return launch_beam_t<C, BList<1>, G, XW>(a, s);
    if (efl <= 128) return launch_beam_t<C, BList<2>, G, XW>(a, s);
    if (efl <= 256) return launch_beam_t<C, BList<4>, G, XW>(a, s);
    constexpr int GW = MH_BEAM_WIDE_G > 0 && MH_BEAM_WIDE_G < G ? MH_BEAM_WIDE_G : G;
    return launch_beam_t<C, BList<8>, GW, XW>(a, s);  // (beam_limits: efl <= 512)
}

template <int L, int V, int XW>
int launch_beam_lds_cfg(const SearchArgs& a, hipStream_t s) {
    if (const int rc = beam_limits(a, true)) return rc;
    return launch_beam_t<Cfg<L, V>, LList, cfg_group<L, V>(), XW>(a, s);
}

// the filtered launch: beam_limits over the route width
template <int L, int V>
int launch_beam_filt_cfg(const SearchArgs& a, const FilterArgs& f, hipStream_t s) {
    if (f.ef < 1 || f.ef > 128 || a.k > f.ef || a.ef < f.ef) return -4;
    if (const int rc = beam_limits(a, true)) return rc;
    const int lds = beam_lds<LList>(a).words;
    return beam_with_screen(a, [&](auto screen) {
        hipLaunchKernelGGL((k_search_beam_filt<Cfg<L, V>, cfg_group<L, V>(), decltype(screen)::value>),
                           dim3((unsigned)a.B), dim3(64), (size_t)4 * (size_t)lds, s, a, f);
        return hipGetLastError() == hipSuccess ? 0 : -1;
    });
}

// the ordered path's pre-pass (k_beam_descend); it fails as the layer-0 launch
// it precedes would (beam_limits)
template <int L, int V>
int launch_beam_descend_cfg(const SearchArgs& a, hipStream_t s) {
    if (const int rc = beam_limits(a, beam_in_lds(a))) return rc;
    const int pvis = beam_desc_vis(a);
    const int lds = pvis > 0 ? pvis : beam_lds<BList<1>>(a).words;  // (the visited set alone)
    return beam_with_screen(a, [&](auto screen) {
        hipLaunchKernelGGL((k_beam_descend<Cfg<L, V>, beam_desc_group<L, V>(), decltype(screen)::value, beam_desc_waves<L, V>()>),
                           dim3((unsigned)a.B), dim3(64), (size_t)4 * (size_t)lds, s, a, pvis);
        return hipGetLastError() == hipSuccess ? 0 : -1;
    });
}

}  // namespace mh
