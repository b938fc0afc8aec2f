// What the two LDS-DMA convolution kernels (conv_igemm_dma.hip, conv3x3_rows.hip) share: the swizzled LDS row, the DMA
// instructions, the counted wait, the scale/shift table's DMA, the XCD-aware block -> tile map, and the once-per-device raise
// of a kernel's dynamic-LDS limit.  (The f16x2 arithmetic they share: f16x2_mma.hpp.)
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>

namespace nbc {
namespace {

typedef __attribute__((ext_vector_type(4))) float f32x4;

// Byte offset of logical 16-byte chunk `chunk` of row `row` in an LDS image of [rows][128 B]: physical slot p of row r holds
// logical chunk p ^ ((r>>1)&7).
__device__ __forceinline__ int lds_off(int row, int chunk) {
  return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4);
}

// One LDS-DMA: 64 lanes x 16 bytes from per-lane global addresses to lds_base .. lds_base+1023.
// M0 carries the wave-uniform LDS base; it is compiler-reserved, so it is saved, written and
// restored inside the one statement that uses it.
__device__ __forceinline__ void dma16(const void* gsrc, unsigned lds_base) {
  unsigned keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %2\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %1, off\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(gsrc), "s"(lds_base)
      : "memory");
}

// The same through a buffer resource: 64 lanes x 16 bytes from `rsrc` base + per-lane 32-bit offset + a
// wave-uniform scalar offset.  Three instructions per DMA instead of seven (no 64-bit pointer per row to
// advance, no M0 save/restore): every instruction a SIMD issues beside its MFMAs costs the matrix pipe
// about its own issue time (tools/mfma_f32_probe.hip).  A lane whose offset lies outside the resource
// (halo and tail lanes: kOutOfRange) gets zeros from the hardware's range check: no zero page.
// M0 is written and left: nothing else in these kernels reads it (the scale/shift DMAs above restore it).
typedef __amdgpu_buffer_rsrc_t rsrc_t;
constexpr unsigned kOutOfRange = 0x80000000u;      // >= every resource size (activations and weights stay below 2 GiB)
__device__ __forceinline__ void dma16_buf(unsigned voff, rsrc_t rsrc, unsigned lds_base, unsigned soff) {
  asm volatile(
      "s_mov_b32 m0, %2\n\t"
      "s_nop 0\n\t"
      "buffer_load_dwordx4 %0, %1, %3 offen lds"
      :
      : "v"(voff), "s"(rsrc), "s"(lds_base), "s"(soff)
      : "memory");
}

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// A block's BN scale/shift pairs (four channels from n0 on per lane of the calling wave) into a 2 KiB LDS table at `lds`, the
// shifts 1024 bytes behind the scales: the epilogue reads them from there, no L2 round trip per 32-pixel slab.
__device__ __forceinline__ void dma_scale_shift(const float* scale, const float* shift, int n0, int lane, unsigned lds) {
  dma16(scale + n0 + lane * 4, lds);
  dma16(shift + n0 + lane * 4, lds + 1024u);
}

// XCD-aware block -> tile map: blocks that share an XCD (block % 8) take a contiguous range of the launch's nblk tiles, so the
// channel tiles of a pixel tile and the halo rows of neighbouring pixel tiles meet in one L2.
__device__ __forceinline__ int xcd_tile(int block, int nblk) {
  const int q = nblk >> 3, rr = nblk & 7, xcd = block & 7;
  return (xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + (block >> 3);
}

// A kernel that asks for more than 64 KiB of dynamic LDS has hipFuncAttributeMaxDynamicSharedMemorySize raised once per device
// (one context per device).  `done` is the kernel's own word, bit d: done on device d; setting it twice from two threads is
// harmless.  *dev: the current device; cus (nullable, [64]): the device's compute units, filled on the same occasion.
inline hipError_t raise_lds_limit_once(std::atomic<unsigned long long>& done, const void* kern, int smem, int* dev, int* cus = nullptr) {
  if (hipGetDevice(dev) != hipSuccess || *dev < 0 || *dev > 63) return hipErrorInvalidDevice;
  if ((done.load(std::memory_order_acquire) >> *dev) & 1ull) return hipSuccess;
  hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, smem);
  if (e != hipSuccess) return e;
  if (cus != nullptr) {
    int n = 0;
    e = hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, *dev);
    if (e != hipSuccess) return e;
    if (n < 1) return hipErrorInvalidDevice;
    cus[*dev] = n;
  }
  done.fetch_or(1ull << *dev, std::memory_order_release);
  return hipSuccess;
}

}  // namespace
}  // namespace nbc
