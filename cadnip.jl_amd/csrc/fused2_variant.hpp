// fused2_variant.hpp -- body of fused2_v<F2_VAR>.hip: instantiates k_fused2<WPB, DC, F2_VAR> (fused2_kernel.hpp) for WPB = 1, 2, 4, 8 and
// both modes (variants 3 and 4, the fixed form and its shape form: transient mode only).  One translation unit per variant, so that the five
// compile in parallel.
#include "fused2_kernel.hpp"

namespace cadnip {

template <> int f2_launch_variant<F2_VAR>(int wpb, bool dc, int grid, size_t shmem, hipStream_t stream, const F2Args& f) {
  return with_wpb(wpb, [&](auto W) {
    constexpr int w = decltype(W)::value;
    if constexpr (F2_VAR == 3 || F2_VAR == 4) return dc ? (int)CADNIP_BADARG : lds_launch(k_fused2<w, false, F2_VAR>, grid, 64 * w, shmem, stream, f);
    else return dc ? lds_launch(k_fused2<w, true, F2_VAR>, grid, 64 * w, shmem, stream, f) : lds_launch(k_fused2<w, false, F2_VAR>, grid, 64 * w, shmem, stream, f);
  });
}

}  // namespace cadnip
