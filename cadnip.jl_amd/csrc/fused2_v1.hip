// fused2_v1.hip -- k_fused2<WPB, DC, 1>: direct residuals, every device type
#define F2_VAR 1
#include "fused2_variant.hpp"
