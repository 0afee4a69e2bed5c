// pixie_amd/csrc/conv_launch.h -- what conv3d_f16x3.hip offers the other translation units next to the pure planner of conv_plan.h:
// the step from a descriptor (and the environment) to the planner's input, and the two tiled launchers.  These need HIP types or
// read the environment, which is why they are not in conv_plan.h.
#pragma once
#include <hip/hip_runtime.h>

#include "conv_plan.h"

namespace pixie {

// the shape fields of a descriptor; flags from which of its optional pointers are set (and the environment, for exact_v1)
ConvShape conv_shape_of(const pixie_conv_desc* d);
bool conv_exact_v1();   // PIXIE_CONV_EXACT_V1 is set: exact-fp32 descriptors go to the first-generation kernel

// pixie_conv3d_forward's two tiled launchers; p = conv_plan(conv_shape_of(d))
int conv3d_f16x3_forward(const pixie_conv_desc* d, const ConvPlan& p, hipStream_t st);
int conv3d_exact_forward(const pixie_conv_desc* d, const ConvPlan& p, hipStream_t st);

}  // namespace pixie
