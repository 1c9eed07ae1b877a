// walks_units.hip -- k_search_compat / k_negatives instantiations (walks.hpp),
// in the units walks_a .. walks_d of units.mk: compiled once per unit with
// -DMH_UNIT=<unit>, each with one group of configurations (engine.hpp
// MH_CFGS_A .. D).
#include "walks.hpp"

#ifndef MH_UNIT
#error "walks_units.hip: compile with -DMH_UNIT=<a unit of units.mk>"
#endif

#define WALKS_(L, V, G)                                                         \
    template int launch_compat_cfg<L, V>(const SearchArgs&, hipStream_t);      \
    template int launch_negatives_cfg<L, V>(const NegArgs&, hipStream_t);

#define U_walks_a MH_CFGS_A(WALKS_)
#define U_walks_b MH_CFGS_B(WALKS_)
#define U_walks_c MH_CFGS_C(WALKS_)
#define U_walks_d MH_CFGS_D(WALKS_)

#define MH_UNIT_CAT2(a, b) a##b
#define MH_UNIT_CAT(a, b) MH_UNIT_CAT2(a, b)

namespace mh {
MH_UNIT_CAT(U_, MH_UNIT)  // (an unknown unit does not compile)
}  // namespace mh
