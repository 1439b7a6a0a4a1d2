// fused2_v0.hip -- k_fused2<WPB, DC, 0>: direct residuals, lean device set (the benchmark's kernel)
#define F2_VAR 0
#include "fused2_variant.hpp"

#ifdef CADNIP_TRACE
// diagnostic library only, not part of include/cadnip_hip.h: the trace counters of this variant, the benchmark's
extern "C" int cadnip_debug_trace(unsigned long long* sum, unsigned long long* cnt, int reset) { return cadnip::trace_read_unit(sum, cnt, reset); }
#endif
