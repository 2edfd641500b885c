// poselib_amd — the host / device function qualifier and the wavefront LDS fence shared by the math headers.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PL_HD __host__ __device__ __forceinline__
// a device function that stays a CALL: for a rarely taken branch whose registers would otherwise be charged to every path of a kernel
#define PL_HD_CALL __host__ __device__ inline __attribute__((noinline))
#define PL_UNROLL _Pragma("unroll") // small constant-trip loops over register arrays: no dynamic indexing -> no scratch
// orders the LDS accesses of the lanes of one wavefront (the hardware executes a wavefront's LDS instructions in order; this keeps the
// compiler from moving or caching accesses across the phases of the algorithm)
#define PL_WAVE_SYNC()                                                                                                 \
    do {                                                                                                               \
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");                                                         \
        __builtin_amdgcn_wave_barrier();                                                                               \
    } while (0)
#else
#define PL_HD inline
#define PL_HD_CALL inline
#define PL_UNROLL
#endif
