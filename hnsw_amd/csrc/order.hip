// order.hip -- the ordered beam search's sort (search_host.cpp, option
// "search_order"): the descent pre-pass's 64-bit path keys into the permutation
// order[B], with rocPRIM's device radix sort.  A unit of its own: the sort's
// templates take as long to compile as a unit of beam_units.hip.
#include <rocprim/device/device_radix_sort.hpp>

#include "engine.hpp"

namespace mh {

// bytes of temporary storage the sort of n keys needs (no launch, no allocation)
int order_sort_temp_bytes(int64_t n, size_t* bytes) {
    *bytes = 0;
    const hipError_t e = rocprim::radix_sort_pairs(nullptr, *bytes, (const unsigned long long*)nullptr,
                                                   (unsigned long long*)nullptr, (const uint32_t*)nullptr,
                                                   (uint32_t*)nullptr, (size_t)n, 0u, 64u, (hipStream_t) nullptr);
    return e == hipSuccess ? 0 : -1;
}

// order[i] = the query at sorted position i (stable: equal keys keep the batch's
// order); bits [0, key_bits) of the keys are compared
int launch_order_sort(const unsigned long long* keys, unsigned long long* keys_sorted, const uint32_t* idx,
                      uint32_t* order, int64_t n, int key_bits, void* temp, size_t temp_bytes, hipStream_t s) {
    if (n <= 0) return 0;
    const unsigned end_bit = (unsigned)(key_bits < 1 ? 1 : key_bits > 64 ? 64 : key_bits);
    const hipError_t e =
        rocprim::radix_sort_pairs(temp, temp_bytes, keys, keys_sorted, idx, order, (size_t)n, 0u, end_bit, s);
    return e == hipSuccess ? 0 : -1;
}

}  // namespace mh
