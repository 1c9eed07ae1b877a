// beam_w2b.hip -- k_search_beam_lds instantiations (beam.hpp: the LDS-resident list,
// max(ef, k) past the register lists) with 2 entries expanded per layer-0 step for 64x4 .. 64x16
#include "beam.hpp"

namespace mh {
template int launch_beam_lds_cfg<64, 4, 2>(const SearchArgs&, hipStream_t);
template int launch_beam_lds_cfg<64, 6, 2>(const SearchArgs&, hipStream_t);
template int launch_beam_lds_cfg<64, 8, 2>(const SearchArgs&, hipStream_t);
template int launch_beam_lds_cfg<64, 12, 2>(const SearchArgs&, hipStream_t);
template int launch_beam_lds_cfg<64, 16, 2>(const SearchArgs&, hipStream_t);
}  // namespace mh
