// build_units.hip -- the insert and delete kernels' explicit instantiations
// (build_compat.hpp, build_batch.hpp, build_link.hpp), in the units of units.mk: compiled once
// per unit with -DMH_UNIT=<unit>, one object each, in parallel.  Each unit holds
// one group of configurations (engine.hpp MH_CFGS_A .. D):
//   build_a .. d       everything but the batched insert's search
//   build_s12a .. d    k_batch_search / k_batch_search_mw, build_expand 1 and 2
//   build_s34a .. d    the same, build_expand 3 and 4
//   build_l12a .. d    k_batch_link (the link pass), build_expand 1 and 2
//   build_l34a .. d    the same, build_expand 3 and 4
#include "build_batch.hpp"
#include "build_link.hpp"
#include "build_compat.hpp"

#ifndef MH_UNIT
#error "build_units.hip: compile with -DMH_UNIT=<a unit of units.mk>"
#endif

#define REST_(L, V, G)                                                                 \
    template int launch_build_compat_cfg<L, V>(const CompatBuildArgs&, int, hipStream_t); \
    template int launch_delete_compat_cfg<L, V>(const DeleteArgs&, hipStream_t);       \
    template int launch_batch_descend_cfg<L, V>(const BatchBuildArgs&, hipStream_t);   \
    template int launch_batch_commit_cfg<L, V>(const BatchBuildArgs&, int64_t, hipStream_t); \
    template int launch_delete_repair_cfg<L, V>(const DeleteArgs&, hipStream_t);
#define S_(L, V, XW) template int launch_batch_search_cfg<L, V, XW>(const BatchBuildArgs&, hipStream_t);
#define S12_(L, V, G) S_(L, V, 1) S_(L, V, 2)
#define S34_(L, V, G) S_(L, V, 3) S_(L, V, 4)
#define K_(L, V, XW) template int launch_batch_link_cfg<L, V, XW>(const BatchBuildArgs&, const LinkArgs&, hipStream_t);
#define K12_(L, V, G) K_(L, V, 1) K_(L, V, 2)
#define K34_(L, V, G) K_(L, V, 3) K_(L, V, 4)

#define U_build_a MH_CFGS_A(REST_)
#define U_build_b MH_CFGS_B(REST_)
#define U_build_c MH_CFGS_C(REST_)
#define U_build_d MH_CFGS_D(REST_)
#define U_build_s12a MH_CFGS_A(S12_)
#define U_build_s12b MH_CFGS_B(S12_)
#define U_build_s12c MH_CFGS_C(S12_)
#define U_build_s12d MH_CFGS_D(S12_)
#define U_build_s34a MH_CFGS_A(S34_)
#define U_build_s34b MH_CFGS_B(S34_)
#define U_build_s34c MH_CFGS_C(S34_)
#define U_build_s34d MH_CFGS_D(S34_)
#define U_build_l12a MH_CFGS_A(K12_)
#define U_build_l12b MH_CFGS_B(K12_)
#define U_build_l12c MH_CFGS_C(K12_)
#define U_build_l12d MH_CFGS_D(K12_)
#define U_build_l34a MH_CFGS_A(K34_)
#define U_build_l34b MH_CFGS_B(K34_)
#define U_build_l34c MH_CFGS_C(K34_)
#define U_build_l34d MH_CFGS_D(K34_)

#define MH_UNIT_CAT2(a, b) a##b
#define MH_UNIT_CAT(a, b) MH_UNIT_CAT2(a, b)

namespace mh {
MH_UNIT_CAT(U_, MH_UNIT)  // (an unknown unit does not compile)
}  // namespace mh
