// beam_desc.hip -- k_beam_descend instantiations (beam.hpp: the ordered path's
// descent pre-pass) for every configuration
#include "beam.hpp"

namespace mh {
#define X_(L, V, G) template int launch_beam_descend_cfg<L, V>(const SearchArgs&, hipStream_t);
MH_FOR_EACH_CFG(X_)
#undef X_
}  // namespace mh
