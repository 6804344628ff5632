// global_mem.h -- plain global-memory accesses for the scene kernels (edit.hip, load.hip, region.hip, volume.hip).
//
// A pointer that reaches a kernel through a struct (DeviceScene, FieldUpdate ...), or an address computed from one, is a generic
// pointer to the compiler: its accesses become flat_* instructions, which also wait on the LDS counter.  Casting to address space 1
// says what every one of these buffers is -- device global memory -- and gives global_* instructions.  The forms below take the
// buffer and an element index (ld32, st32, ldi32, ld8, st8, ld64, st64) or a byte offset (ld128, st128: any 16-byte aligned place
// of a buffer of bytes or words).  trace.hip, traverse.h, wavefront.hip and query.hip have accessors of their own.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace bm {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) uint8_t g_u8;
typedef __attribute__((address_space(1))) uint32_t g_u32;
typedef __attribute__((address_space(1))) int32_t g_i32;
typedef __attribute__((address_space(1))) uint64_t g_u64;
typedef __attribute__((address_space(1))) u32x4 g_u32x4;

__device__ __forceinline__ uint32_t ld8(const uint8_t* p, size_t i) { return ((const g_u8*)p)[i]; }
__device__ __forceinline__ void st8(uint8_t* p, size_t i, uint32_t v) { ((g_u8*)p)[i] = static_cast<uint8_t>(v); }
__device__ __forceinline__ uint32_t ld32(const uint32_t* p, size_t i) { return ((const g_u32*)p)[i]; }
__device__ __forceinline__ void st32(uint32_t* p, size_t i, uint32_t v) { ((g_u32*)p)[i] = v; }
__device__ __forceinline__ int32_t ldi32(const int32_t* p, size_t i) { return ((const g_i32*)p)[i]; }
__device__ __forceinline__ uint64_t ld64(const uint64_t* p, size_t i) { return ((const g_u64*)p)[i]; }
__device__ __forceinline__ void st64(uint64_t* p, size_t i, uint64_t v) { ((g_u64*)p)[i] = v; }
// byte offsets are signed: a region's volume offset is relative to a box corner that may lie outside the world
__device__ __forceinline__ u32x4 ld128(const void* p, int64_t byte) { return *(const g_u32x4*)((const g_u8*)p + byte); }
__device__ __forceinline__ void st128(void* p, int64_t byte, u32x4 v) { *(g_u32x4*)((g_u8*)p + byte) = v; }

} // namespace bm
