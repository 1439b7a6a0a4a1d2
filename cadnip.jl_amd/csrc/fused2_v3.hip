// fused2_v3.hip -- k_fused2<WPB, false, 3>: variant 0 with the default transient call's switches fixed at compile time (lds_layout.hpp: f2_fixed_ok)
#define F2_VAR 3
#include "fused2_variant.hpp"
