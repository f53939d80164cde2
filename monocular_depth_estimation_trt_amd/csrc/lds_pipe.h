// The primitives a global -> LDS software pipeline rests on: the 16-byte
// LDS-DMA, the counted vmcnt wait, the raw workgroup barrier and the row
// swizzle.  One definition each; a new pipelined kernel takes them from here.
// Each of the DMA and the wait has two forms, which differ in what hipcc's
// wait insertion sees -- the comments say when a kernel needs which.  A kernel
// is never switched from one form to the other without re-reading its ISA.
#pragma once
#include "mde_device.h"

namespace mde {

// 16-byte LDS-DMA (global_load_lds_dwordx4, 64-bit vaddr form, no VGPR round
// trip): lane l's 16 bytes at src land at lds_wave_base + 16 l -- the LDS
// image of a wave-instruction is lane-linear, so a swizzle goes on the SOURCE
// address.  A lane cannot be masked, it can be redirected (padding taps read a
// zero line).  The compiler sees this one: while one is pending, the lgkmcnt
// waits it places for ds_reads are lgkmcnt(0) (see glds16_asm).
MDE_DEV void glds16(const void* src, void* lds_wave_base) {
  __builtin_amdgcn_global_load_lds(src, lds_wave_base, 16, 0, 0);
}

// The same LDS-DMA (64-bit vaddr form) issued from inline asm: hipcc does not
// see it, so its ds_read waits in the DMA's shadow stay counted (lgkmcnt(N))
// instead of lgkmcnt(0) -- it models a pending FLAT LDS-DMA as an
// out-of-order lgkm event.  The caller counts the DMA itself (vmcnt) and
// orders LDS accesses around it with "memory" asm.  M0 is written and
// restored inside the statement (compiler-reserved).
MDE_DEV void glds16_asm(const void* src, unsigned lds_dst) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(src), "s"(lds_dst)
               : "memory");
}

// s_waitcnt vmcnt(N) as opaque asm: all but the N youngest of this wave's
// loads / LDS-DMAs have landed (N = 0: drained).  The compiler's own wait
// insertion does not know of it and still places its waits as if nothing had
// been waited for: the form for a ring whose only loads in flight across the
// wait are LDS-DMAs (otherwise wait_vm_seen).  N = 0 is spelled without an
// operand: the same instruction text, but to the optimiser an asm statement
// with an immediate operand is a different statement where it merges code
// paths, and conv.hip without its weight loads (tools/ablate.py conv_now)
// compiled to other code with the operand form.
template <int N>
MDE_DEV void wait_vm_n() {
  if constexpr (N == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// s_waitcnt vmcnt(N) as an instruction the compiler's wait insertion sees
// (an asm wait is opaque to it: loads it thinks pending at the loop head get
// a vmcnt(0) at their first use in EVERY unit -- with the W chunk DMA issued
// just before, that drained the panel GEMM's ring each unit).  For a kernel
// that keeps register loads in flight across its counted waits.  N < 64;
// expcnt / lgkmcnt not waited.  gfx9 simm16: vmcnt [3:0] + [15:14],
// expcnt [6:4] = 7, lgkmcnt [11:8] = 15
template <int N>
MDE_DEV void wait_vm_seen() {
  static_assert(N >= 0 && N < 64, "vmcnt");
  __builtin_amdgcn_s_waitcnt((N & 15) | ((N >> 4) << 14) | 0x0F70);
}

// Workgroup barrier that leaves LDS-DMA in flight (__syncthreads() would
// also drain vmcnt, i.e. the ring's loads and an epilogue's global stores):
// own LDS accesses retired, raw s_barrier, and compiler fences so no LDS
// access moves across it.
MDE_DEV void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// Physical 16-byte chunk of logical chunk `chunk` in row `row` of a 128-byte-
// row LDS image whose ds_read_b128 lane groups take consecutive rows at one
// logical chunk (the 16x16x32 fragment reads): 8 rows over 8 chunks, conflict-
// free.  Applied on the DMA's source address and on the fragment read.
// (Reads that take rows of both parities per lane group swizzle by
// (row >> 1) instead: attention.hip's swz, the 64-byte-row cpch<32>.)
MDE_DEV int swz7(int row, int chunk) { return chunk ^ (row & 7); }

}  // namespace mde
