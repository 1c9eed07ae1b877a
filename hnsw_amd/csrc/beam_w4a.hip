// beam_w4a.hip -- k_search_beam_lds instantiations (beam.hpp: the LDS-resident list,
// max(ef, k) past the register lists) with 4 entries expanded per layer-0 step for 16x1 .. 64x3
#include "beam.hpp"

namespace mh {
template int launch_beam_lds_cfg<16, 1, 4>(const SearchArgs&, hipStream_t);
template int launch_beam_lds_cfg<32, 1, 4>(const SearchArgs&, hipStream_t);
template int launch_beam_lds_cfg<64, 1, 4>(const SearchArgs&, hipStream_t);
template int launch_beam_lds_cfg<64, 2, 4>(const SearchArgs&, hipStream_t);
template int launch_beam_lds_cfg<64, 3, 4>(const SearchArgs&, hipStream_t);
}  // namespace mh
