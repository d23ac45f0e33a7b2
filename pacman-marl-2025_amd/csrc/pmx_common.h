// pmx_common.h -- what the network kernels' files (pmx_train, pmx_actor, pmx_critic, pmx_heads, pmx_actor_head) share: the host
// helpers of their launchers and the few device helpers more than one of them uses.  Internal: not part of the C ABI of
// include/pmx.h.  A helper that one file alone uses stays in that file.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>
#include <set>
#include <utility>

#include "../../include/pmx.h"

// ---------------------------------------------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------------------------------------------
// the status of a launcher: whatever the launches since the last call left behind
inline int pmx_launch_rc() { return hipGetLastError() == hipSuccess ? PMX_OK : PMX_ERR_HIP; }

// compute units of the CURRENT device (asked on every call: the caller may have switched devices); 256 when the runtime will not say
inline int pmx_cu_count()
{
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus = 256;
    return cus;
}

// A launch with more than 64 KB of dynamic LDS needs hipFuncAttributeMaxDynamicSharedMemorySize raised first.  The attribute belongs
// to ONE kernel on the CURRENT device, so it is set once per (kernel address, device); the forward thread and autograd's backward
// worker both come through here, hence the lock.  limit: what to ask for (PMX_LDS_PER_CU less the kernel's static LDS).
constexpr size_t PMX_LDS_PER_CU = 160 * 1024;
inline int pmx_allow_lds(const void *fn, size_t lds, size_t limit)
{
    if (lds <= 65536) return PMX_OK;
    static std::mutex mu;
    static std::set<std::pair<const void *, int>> done;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return PMX_ERR_HIP;
    std::lock_guard<std::mutex> lock(mu);
    if (done.count({fn, dev})) return PMX_OK;
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)limit) != hipSuccess) return PMX_ERR_HIP;
    done.insert({fn, dev});
    return PMX_OK;
}

// Partial-row gradient buffers (pmx_critic.hip owns the state behind pmx_defer_row_sums / pmx_last_partial_rows).  A backward entry
// point whose kernel left `rows` partial rows in rows 1 .. rows of grad ends with pmx_finish_partial_rows: it records rows for
// pmx_last_partial_rows and, unless the sums are deferred or rows == 0, launches the row sum into row 0 on st.  An entry point that
// wrote row 0 directly says pmx_no_partial_rows.
int pmx_finish_partial_rows(float *grad, int rows, int floats, hipStream_t st);
void pmx_no_partial_rows();

// ---------------------------------------------------------------------------------------------------------------
// Device side
// ---------------------------------------------------------------------------------------------------------------
// MFMA operands (bf16 travels as short) and accumulators
typedef __attribute__((ext_vector_type(8))) short bf16x8;
typedef __attribute__((ext_vector_type(4))) short bf16x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;

// two floats -> packed bf16 (a low, b high), round to nearest even: one v_cvt_pk_bf16_f32
__device__ __forceinline__ uint32_t bf_pack(float a, float b)
{
    const f32x2 f = {a, b};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(f, bf16x2_t));
}
// a float rounded to bf16, as a float
__device__ __forceinline__ float bf_round(float x) { return __uint_as_float(bf_pack(x, 0.f) << 16); }
__device__ __forceinline__ float bf_lo(uint32_t u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bf_hi(uint32_t u) { return __uint_as_float(u & 0xFFFF0000u); }

// sum over the 64 lanes of a wavefront, in every lane
__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// GELU, the exact erf form (nn.GELU() default), and its derivative
__device__ __forceinline__ float gelu_exact(float z) { return 0.5f * z * (1.0f + erff(z * 0.70710678118654752f)); }
__device__ __forceinline__ float gelu_grad(float z)
{
    return 0.5f * (1.0f + erff(z * 0.70710678118654752f)) + z * 0.3989422804014327f * __expf(-0.5f * z * z);
}
