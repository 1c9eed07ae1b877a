// beam_units.hip -- the beam search's explicit instantiations (beam.hpp), in
// the units of units.mk: compiled once per unit with -DMH_UNIT=<unit>, one
// object each, so that the units compile in parallel.
//   beam_a .. beam_d       k_search_beam, the standard search (XW 1), one group
//                          of configurations each (engine.hpp MH_CFGS_A .. D)
//   beam_x2a/b, beam_x4a/b k_search_beam with 2 / 4 entries expanded per
//                          layer-0 step (search_expand), groups A B / C D
//   beam_w1a/b .. w4a/b    k_search_beam_lds (the LDS-resident list, max(ef, k)
//                          past the register lists), XW 1 / 2 / 4, groups A B / C D
//   beam_fa, beam_fb       k_search_beam_filt (the filtered search), groups A B / C D
//   beam_desc              k_beam_descend (the ordered path's descent pre-pass),
//                          every configuration
#include "beam.hpp"

#ifndef MH_UNIT
#error "beam_units.hip: compile with -DMH_UNIT=<a unit of units.mk>"
#endif

#define REG1_(L, V, G) template int launch_beam_cfg<L, V, 1>(const SearchArgs&, hipStream_t);
#define REG2_(L, V, G) template int launch_beam_cfg<L, V, 2>(const SearchArgs&, hipStream_t);
#define REG4_(L, V, G) template int launch_beam_cfg<L, V, 4>(const SearchArgs&, hipStream_t);
#define LDS1_(L, V, G) template int launch_beam_lds_cfg<L, V, 1>(const SearchArgs&, hipStream_t);
#define LDS2_(L, V, G) template int launch_beam_lds_cfg<L, V, 2>(const SearchArgs&, hipStream_t);
#define LDS4_(L, V, G) template int launch_beam_lds_cfg<L, V, 4>(const SearchArgs&, hipStream_t);
#define FILT_(L, V, G) template int launch_beam_filt_cfg<L, V>(const SearchArgs&, const FilterArgs&, hipStream_t);
#define DESC_(L, V, G) template int launch_beam_descend_cfg<L, V>(const SearchArgs&, hipStream_t);

#define U_beam_a MH_CFGS_A(REG1_)
#define U_beam_b MH_CFGS_B(REG1_)
#define U_beam_c MH_CFGS_C(REG1_)
#define U_beam_d MH_CFGS_D(REG1_)
#define U_beam_x2a MH_CFGS_A(REG2_) MH_CFGS_B(REG2_)
#define U_beam_x2b MH_CFGS_C(REG2_) MH_CFGS_D(REG2_)
#define U_beam_x4a MH_CFGS_A(REG4_) MH_CFGS_B(REG4_)
#define U_beam_x4b MH_CFGS_C(REG4_) MH_CFGS_D(REG4_)
#define U_beam_w1a MH_CFGS_A(LDS1_) MH_CFGS_B(LDS1_)
#define U_beam_w1b MH_CFGS_C(LDS1_) MH_CFGS_D(LDS1_)
#define U_beam_w2a MH_CFGS_A(LDS2_) MH_CFGS_B(LDS2_)
#define U_beam_w2b MH_CFGS_C(LDS2_) MH_CFGS_D(LDS2_)
#define U_beam_w4a MH_CFGS_A(LDS4_) MH_CFGS_B(LDS4_)
#define U_beam_w4b MH_CFGS_C(LDS4_) MH_CFGS_D(LDS4_)
#define U_beam_fa MH_CFGS_A(FILT_) MH_CFGS_B(FILT_)
#define U_beam_fb MH_CFGS_C(FILT_) MH_CFGS_D(FILT_)
#define U_beam_desc MH_FOR_EACH_CFG(DESC_)

#define MH_UNIT_CAT2(a, b) a##b
#define MH_UNIT_CAT(a, b) MH_UNIT_CAT2(a, b)

namespace mh {
MH_UNIT_CAT(U_, MH_UNIT)  // (an unknown unit does not compile)
}  // namespace mh
