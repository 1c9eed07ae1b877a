// build.hip -- the insert and delete entry points: each picks the launcher of
// the index's dimension configuration.  The kernels are in build_compat.hpp (the
// reference's sequential walks) and build_batch.hpp (the throughput insert).
#include "build_batch.hpp"
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

int launch_delete_compat(const DeleteArgs& a, int lpr, int vpl, hipStream_t s) {
    if (a.nids <= 0) return 0;
    return with_cfg(lpr, vpl, [&](auto c) { return launch_delete_compat_cfg<c.L, c.V>(a, s); });
}

int launch_delete_repair(const DeleteArgs& a, int lpr, int vpl, hipStream_t s) {
    if (a.n <= 0) return 0;
    return with_cfg(lpr, vpl, [&](auto c) { return launch_delete_repair_cfg<c.L, c.V>(a, s); });
}

}  // namespace mh
