// fused2_v2.hip -- k_fused2<WPB, DC, 2>: assembled residual r = J u + C beta - b (diagnostic, CADNIP_F2_NODIRECT=1), every device type
#define F2_VAR 2
#include "fused2_variant.hpp"
