// fused2_v4.hip -- k_fused2<WPB, false, 4>: variant 3 with the circuit's block list fixed to the CMOS-cell shape as well (lds_layout.hpp: f2_shape_ok)
#define F2_VAR 4
#include "fused2_variant.hpp"
