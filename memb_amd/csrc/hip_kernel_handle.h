// What memb_hip.hip needs of a kernel of another translation unit to launch it: the handle every selector of the
// hip_<family>.h headers returns, and the number of blocks of a grid whose wavefronts own a run of items each. Plain C++:
// the planning programs under tests/cpp/ see it through those headers, without the HIP runtime.
#pragma once

#include <cstdint>

namespace memb {

struct KernelHandle {
    const void* address;   // host address for hipLaunchKernel / hipFuncGetAttributes; null where no instance exists
    const char* name;      // the kernel family, or the instance where the selector knows it: error messages, *_kernel_name
};

// Blocks of `waves` wavefronts that own perWave consecutive items each, over count >= 1 items (0 counts as 1 in either
// factor). 0: too many for one launch.
inline uint32_t gridBlocks(uint32_t waves, uint32_t perWave, uint64_t count)
{
    const uint64_t perBlock = uint64_t(waves ? waves : 1) * (perWave ? perWave : 1);
    const uint64_t blocks = (count + perBlock - 1) / perBlock;
    return blocks >= 0x7FFFFFFFull ? 0 : static_cast<uint32_t>(blocks);
}

}  // namespace memb
