// fused_team.hip -- instantiates k_fteam<NW> (fused_team_kernel.hpp): the fused Newton kernel with a team of NW waves per sweep instance.
#include "fused_team_kernel.hpp"

namespace cadnip {

int fteam_launch(int nw, int grid, size_t shmem, hipStream_t stream, const F2Args& f) {
  return nw == 4 ? lds_launch(k_fteam<4, false>, grid, 256, shmem, stream, f) : lds_launch(k_fteam<2, false>, grid, 128, shmem, stream, f);
}

int fteam_launch_step(int grid, size_t shmem, hipStream_t stream, const F2Args& f) { return lds_launch(k_fteam<4, true>, grid, 256, shmem, stream, f); }

#ifdef CADNIP_TRACE
int trace_read_team(unsigned long long* sum, unsigned long long* cnt, int reset, int wave) {
  TRY_RC(trace_read_unit(sum, cnt, reset));
  HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_trace_wave), &wave, sizeof(int)));
  return CADNIP_OK;
}
#endif

}  // namespace cadnip

#ifdef CADNIP_TRACE
// diagnostic library only: cycle timeline of wave `wave` of the first team (tools/trace_fused2.py --team)
extern "C" int cadnip_debug_trace_team(unsigned long long* sum, unsigned long long* cnt, int reset, int wave) { return cadnip::trace_read_team(sum, cnt, reset, wave); }
#endif
