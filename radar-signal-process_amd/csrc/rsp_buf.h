// Raw buffer access for gfx950 (device code only).
//
// A buffer resource (V#) covers one CPI plane; lanes address it with a 32-bit per-lane
// voffset plus a wave-uniform soffset, so strided slow-time / Doppler-row accesses put
// their row stride in an SGPR and spend no VALU on 64-bit address arithmetic.  The
// hardware range check (offset >= num_records) makes loads return 0 and drops stores,
// which replaces per-element `if (in range)` branches: a lane that must not touch memory
// uses kOob as its voffset.
#pragma once
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rsp {

constexpr int kBufWord3 = 0x00020000;    // gfx9 resource word 3 (raw, 32-bit data format)
constexpr uint32_t kOob = 0x80000000u;   // voffset beyond any plane (planes are < 2 GiB)

__device__ __forceinline__ __amdgpu_buffer_rsrc_t buf_rsrc(const void* base, uint32_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)bytes, kBufWord3);
}

__device__ __forceinline__ float2 buf_ld_f2(__amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff) {
    return __builtin_bit_cast(float2, __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, 0));
}
__device__ __forceinline__ float buf_ld_f(__amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0));
}
__device__ __forceinline__ void buf_st_f2(float2 v, __amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff) {
    typedef int v2i __attribute__((ext_vector_type(2)));
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2i, v), r, voff, soff, 0);
}
__device__ __forceinline__ void buf_st_f(float v, __amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff) {
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, v), r, voff, soff, 0);
}
__device__ __forceinline__ void buf_st_u8(uint8_t v, __amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff) {
    __builtin_amdgcn_raw_buffer_store_b8(v, r, voff, soff, 0);
}

// Cache policy of the streamed-once planes (echo input, RDM output): the default.  Marking
// them non-temporal (aux bit 1, `nt`) so they would not evict the PC scratch was measured
// slower (the range stage re-reads RDM neighbourhoods, and PC gains nothing).
constexpr int kStreamAux = 0;

// one complex element of an input plane (complex fp32, or fp16 I/Q widened on load).  The fp16
// echo (config c5: 512 x 16384, a 67 MB PC scratch per CPI and pipeline, near the 256 MB
// Infinity Cache with two pipelines) is loaded non-temporal (aux bit 1, `nt`): read once, it
// then evicts less of the scratch (c5 +2 %).  The same hint on the fp32 echo was neutral at c3
// and cost c4 3 %, and on the MTD's scratch loads cost c3 2 % and c5 2 %.
constexpr int kEchoF16Aux = 2;
__device__ __forceinline__ float2 buf_ld_c(const float2*, __amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff) {
    return __builtin_bit_cast(float2, __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, kStreamAux));
}
__device__ __forceinline__ float2 buf_ld_c(const __half2*, __amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff) {
    return __half22float2(__builtin_bit_cast(__half2, __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, kEchoF16Aux)));
}
// the same through a plain pointer (complex fp64 narrowed: the host-layout conversions)
__device__ __forceinline__ float2 ld_c(const float2* p) { return *p; }
__device__ __forceinline__ float2 ld_c(const __half2* p) { return __half22float2(*p); }
__device__ __forceinline__ float2 ld_c(const double2* p) {
    double2 d = *p;
    return make_float2((float)d.x, (float)d.y);
}
// streamed-once store (RDM)
__device__ __forceinline__ void buf_st_f_stream(float v, __amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff) {
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, v), r, voff, soff, kStreamAux);
}

}  // namespace rsp
