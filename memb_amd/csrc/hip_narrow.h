// The kernels of memb_hip_narrow.hip (bf16 / fp16 rows) as memb_hip.hip launches them (hip_kernel_table.h: launchKernelAddress; hip_decode_launch.h: launchRowwise):
// host addresses for hipLaunchKernel / hipFuncGetAttributes. Their parameters are the TrainedParams / UniformParams / FullParams of the device
// headers, which both translation units include.
#pragma once

namespace memb_narrow {

// decode_trained_narrow<HAS_SUB, MODE, FAST, OUT> for MODE OUT_SCALAR, OUT_VEC4, OUT_FLAT and outType MEMB_HIP_OUT_BF16 /
// MEMB_HIP_OUT_F16; null where no instance exists (HAS_SUB with FAST, another mode or type)
const void* trainedKernel(bool hasSub, int mode, bool fast, int outType);
// dequant_uniform_narrow<VEC4, OUT> / gather_full_narrow<VEC4, OUT>
const void* uniformKernel(bool vec4, int outType);
const void* fullKernel(bool vec4, int outType);

}  // namespace memb_narrow
