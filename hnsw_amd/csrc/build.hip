// build.hip -- the insert and delete entry points: each picks the launcher of
// the index's dimension configuration.  The kernels are in build_compat.hpp (the
// reference's sequential walks), build_batch.hpp (the throughput insert) and
// build_link.hpp (its link pass).
#include "build_batch.hpp"
#include "build_link.hpp"
#include "build_compat.hpp"

namespace mh {
// instantiated in the units of build_units.hip
#define X_(L, V, G)                                                                           \
    extern template int launch_build_compat_cfg<L, V>(const CompatBuildArgs&, int, hipStream_t); \
    extern template int launch_delete_compat_cfg<L, V>(const DeleteArgs&, hipStream_t);       \
    extern template int launch_batch_descend_cfg<L, V>(const BatchBuildArgs&, hipStream_t);   \
    extern template int launch_batch_search_cfg<L, V, 1>(const BatchBuildArgs&, hipStream_t); \
    extern template int launch_batch_search_cfg<L, V, 2>(const BatchBuildArgs&, hipStream_t); \
    extern template int launch_batch_search_cfg<L, V, 3>(const BatchBuildArgs&, hipStream_t); \
    extern template int launch_batch_search_cfg<L, V, 4>(const BatchBuildArgs&, hipStream_t); \
    extern template int launch_batch_commit_cfg<L, V>(const BatchBuildArgs&, int64_t, hipStream_t); \
    extern template int launch_batch_link_cfg<L, V, 1>(const BatchBuildArgs&, const LinkArgs&, hipStream_t); \
    extern template int launch_batch_link_cfg<L, V, 2>(const BatchBuildArgs&, const LinkArgs&, hipStream_t); \
    extern template int launch_batch_link_cfg<L, V, 3>(const BatchBuildArgs&, const LinkArgs&, hipStream_t); \
    extern template int launch_batch_link_cfg<L, V, 4>(const BatchBuildArgs&, const LinkArgs&, hipStream_t); \
    extern template int launch_delete_repair_cfg<L, V>(const DeleteArgs&, hipStream_t);
MH_FOR_EACH_CFG(X_)
#undef X_

int launch_build_compat(const CompatBuildArgs& a, int lpr, int vpl, int waves, hipStream_t s) {
    return with_cfg(lpr, vpl, [&](auto c) { return launch_build_compat_cfg<c.L, c.V>(a, waves, s); });
}

int launch_build_batch_descend(const BatchBuildArgs& a, int lpr, int vpl, hipStream_t s) {
    return with_cfg(lpr, vpl, [&](auto c) { return launch_batch_descend_cfg<c.L, c.V>(a, s); });
}

// f(std::integral_constant<int, XW>()) for the option build_expand (2, 3, 4, else the standard 1)
template <class F>
static int with_build_expand(int expand, F&& f) {
    return expand == 4   ? f(std::integral_constant<int, 4>())
           : expand == 3 ? f(std::integral_constant<int, 3>())
           : expand == 2 ? f(std::integral_constant<int, 2>())
                         : f(std::integral_constant<int, 1>());
}

int launch_build_batch_search(const BatchBuildArgs& a, int lpr, int vpl, hipStream_t s) {
    return with_build_expand(a.expand, [&](auto xw) {
        return with_cfg(lpr, vpl, [&](auto c) { return launch_batch_search_cfg<c.L, c.V, xw.value>(a, s); });
    });
}

int launch_build_batch_commit(const BatchBuildArgs& a, int lpr, int vpl, int64_t max_touched, hipStream_t s) {
    if (max_touched <= 0) return 0;
    return with_cfg(lpr, vpl, [&](auto c) { return launch_batch_commit_cfg<c.L, c.V>(a, max_touched, s); });
}

int launch_build_batch_link(const BatchBuildArgs& a, const LinkArgs& k, int lpr, int vpl, hipStream_t s) {
    return with_build_expand(a.expand, [&](auto xw) {
        return with_cfg(lpr, vpl, [&](auto c) { return launch_batch_link_cfg<c.L, c.V, xw.value>(a, k, s); });
    });
}

// One wave per batch row of the layer: a staged row replaces the row in the
// adjacency (after k_batch_link has finished: nobody reads the layer now).
// Two batch-mates can select each other: u's staged row then holds v while v's
// proposal to u waits in u's slots.  k_batch_commit ranks the row and the
// proposals as one set and takes no entry twice, so the staged entries that a
// stored proposal repeats are left to the proposal (the same distance: d(u, v)
// == d(v, u) bitwise); the row keeps its order.
__global__ __launch_bounds__(64) void k_batch_link_apply(LinkKernelArgs ka) {
    const BatchBuildArgs& a = ka.a;
    const LinkArgs& k = ka.k;
    uint32_t u;
    if (!batch_node(a, u)) return;
    const int l = a.layer;
    if (a.levels[u] < l) return;
    const int lane = lane_id();
    const int64_t slot = (int64_t)u - a.n0;
    const int capl = a.g.layers[l].cap;
    const int nd = min(k.deg[slot], min(min(capl, k.stride), 64));
    if (nd < 0) return;
    const int nin = min(a.inc_cnt[u], a.inc_cap);
    int32_t c = -1;
    float d = 0.f;
    bool keep = lane < nd;
    if (keep) {
        c = k.adj[(size_t)slot * k.stride + lane];
        d = k.adjd[(size_t)slot * k.stride + lane];
        for (int j = 0; j < nin; ++j) keep = keep && a.inc_src[(size_t)u * a.inc_cap + j] != (uint32_t)c;
    }
    const unsigned long long m = __ballot(keep);
    if (keep) {
        const int e = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0));
        a.g.layers[l].adj[(size_t)u * capl + e] = c;
        a.g.layers[l].adjd[(size_t)u * capl + e] = d;
    }
    if (lane == 0) a.g.layers[l].deg[u] = __popcll(m);
}

int launch_build_batch_link_apply(const BatchBuildArgs& a, const LinkArgs& k, hipStream_t s) {
    const int64_t n = a.order ? a.count : a.n1 - a.n0;
    if (n <= 0) return 0;
    return launch_grid(k_batch_link_apply, n, 64, 0, LinkKernelArgs{a, k}, s);
}

int launch_delete_compat(const DeleteArgs& a, int lpr, int vpl, hipStream_t s) {
    if (a.nids <= 0) return 0;
    return with_cfg(lpr, vpl, [&](auto c) { return launch_delete_compat_cfg<c.L, c.V>(a, s); });
}

int launch_delete_repair(const DeleteArgs& a, int lpr, int vpl, hipStream_t s) {
    if (a.n <= 0) return 0;
    return with_cfg(lpr, vpl, [&](auto c) { return launch_delete_repair_cfg<c.L, c.V>(a, s); });
}

}  // namespace mh
