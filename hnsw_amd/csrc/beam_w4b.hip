// beam_w4b.hip -- k_search_beam_lds instantiations (beam.hpp: the LDS-resident list,
// max(ef, k) past the register lists) with 4 entries expanded per layer-0 step for 64x4 .. 64x16
#include "beam.hpp"

namespace mh {
template int launch_beam_lds_cfg<64, 4, 4>(const SearchArgs&, hipStream_t);
template int launch_beam_lds_cfg<64, 6, 4>(const SearchArgs&, hipStream_t);
template int launch_beam_lds_cfg<64, 8, 4>(const SearchArgs&, hipStream_t);
template int launch_beam_lds_cfg<64, 12, 4>(const SearchArgs&, hipStream_t);
template int launch_beam_lds_cfg<64, 16, 4>(const SearchArgs&, hipStream_t);
}  // namespace mh
