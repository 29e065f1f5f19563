// resource usage of k_skpart_w alone: quick register / LDS checks while reshaping the partition
// kernel, without compiling assemble.hip.  From the repository root:
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -munsafe-fp-atomics --cuda-device-only -c \
//       -Rpass-analysis=kernel-resource-usage -o /dev/null tools/micro/skpart_tu.hip
// The headline's forms (k = 31, 100-base reads: 7 staged KiB, W = 17, runs of 17 windows whole)
// with and without the input check, and the plain W = 17 form of reads past 128 windows.
#include "../../pycuda-euler_amd/csrc/common.h"
#include "../../pycuda-euler_amd/csrc/count_sk2.h"
#define SKPART_TU(NPF, W, VAL, N17)                                                                               \
    template __global__ void ec::k_skpart_w<NPF, W, VAL, N17>(                                                    \
        const uint8_t *__restrict__, const uint64_t *__restrict__, uint64_t, ec::MinCfg, uint32_t, uint64_t,      \
        uint32_t, uint64_t, uint32_t, uint4 *, unsigned int *, uint8_t *, unsigned long long *, unsigned int *,   \
        unsigned int *, unsigned long long *, uint32_t, uint32_t);
SKPART_TU(7, 17, true, true)
SKPART_TU(7, 17, false, true)
SKPART_TU(7, 17, true, false)
