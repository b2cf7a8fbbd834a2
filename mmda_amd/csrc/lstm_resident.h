// biLSTM / biGRU recurrence with W_hh RESIDENT ON CHIP (bf16 mode) - the fast path behind mmda_lstm_fwd / mmda_lstm_bwd: what the kernel
// files lstm_barrier.hip, lstm_wave.hip, lstm_quad.hip and the host side lstm_resident.hip (plan_resident() picks the form) share.
// lstm.hip re-streams W_hh (720 KB bf16 for the 300-wide text LSTM) from L2 through one CU on every one of the 2*T dependent steps;
// that stream, not the matrix cores, sets its step time.  Here the 16-unit hidden tiles of one (modality, direction, 32-sample batch
// group) are split over a CLUSTER of workgroups that keep their part of W_hh on chip for the whole sequence, so a step is: MFMA +
// lane-local cell update + one exchange inside the cluster (forward: all-gather of the new h; backward: reduce-scatter of dh).
//
// Exchange protocol (MI355X guide, Guideline 16, form R1), common part: handed-off bytes leave as agent-scope write-through (sc1)
// stores and are read by L1-bypassing (sc1) loads, so no acquire fence is needed (plain stores where the waves verified that their
// cluster shares an XCD: Wave, Quad).  Epochs are monotonic across steps AND launches (base passed by the host): nothing is reset.
// X is double buffered by epoch parity (an image is overwritten two epochs later, after every consumer has signalled the epoch in
// between).  Every spin is BOUNDED: a timed-out poll sets a sticky abort word and the grid always drains.  All workgroups of a
// launch are co-resident: the host caps a launch and chunks larger batches.  How a consumer learns that the bytes are there:
//   barrier + flag (Barrier, some H > 320; a workgroup = 2 hidden tiles x 2 m-tiles, W_hh in LDS)  producer: own slice -> X; EVERY
//       storing wave drains (s_waitcnt vmcnt(0)); workgroup barrier; ONE lane stores flag[workgroup] = epoch.  consumer: ONE wave
//       polls the other NC-1 flags (lane per producer, s_sleep); workgroup barrier; the loads land in LDS.
//   per-wave flag (Wave, every H <= 320; a wave = one (m-tile, hidden tile), W_hh in registers, 1, 2 or 4 waves per block)  the wave
//       stores its tile, drains, raises ITS OWN flag; lane tau of a consumer polls the flag of tile tau.  No workgroup barrier.
//   data-tagged (Quad, as Wave + gate-minor + all tiles resident; four waves per tile split the step)  steps 0..2 by per-wave
//       flag; then bit 14 of every published bf16 (free: |value| < 2) carries bit 1 of the epoch and consumers poll the data itself.
#pragma once
#include "common.h"
#include "internal.h"

// A named namespace: CLaunch is the parameter of every kernel and of the `Kernel` pointers the kernel files hand to
// lstm_resident.hip, and a struct of an anonymous namespace would be a different type in every translation unit.  With one type
// the host keeps its typed launch (hipLaunchKernelGGL); `const void*` + hipLaunchKernel would pass an unchecked argument array.
namespace mmda_resident {

constexpr int GROUP = 32;            // samples per cluster (two 16-row MFMA tiles)
constexpr int MAXD = 4;
constexpr unsigned SPIN_LIMIT = 1u << 20;
constexpr int MAXB = 1024;           // blocks per launch (the four-waves-per-tile kernels share CUs: up to 4 blocks each)
constexpr int QUAD_LDS = 2 * 4 * 16 * 16 * 4 * 4;      // Quad, bytes: parity x source wave x 16 rows x 16 units x 4 gates, fp32

typedef unsigned long long u64;
typedef __attribute__((address_space(1))) u64 gu64;
typedef __attribute__((address_space(1))) unsigned gu32;

struct CDesc {
  int H, Hp, Kp, KS, KSB, nHT, TPW, NC;
  float* gates; float* cstash; float* hseq; const void* wpack[2]; const void* wpack_c[2]; float* utt; int layer;
  void* dg16;                        // backward, optional: bf16 copy of the gate gradients (gate-minor wave kernel only)
  int dg16_only;                     // ... and no fp32 store of them
  const float* d_hseq;
  unsigned char* xchg;
  int wg_begin;
  int NCw;                           // wave-autonomous forward: workgroups per cluster = ceil(2 * nHT / waves per block)
};
struct CLaunch {
  CDesc d[MAXD];
  int n, B, T, g0, ng;               // batch groups [g0, g0+ng) of this launch
  const int32_t* lengths;
  unsigned epoch_base;
  unsigned long long* dbg;           // diagnostics only: per-workgroup phase cycle sums (NULL in production)
  int gate_minor;                    // `gates` columns are [dir][unit][gate]: 16-byte accesses (see mmda_lstm_desc)
  int xcd_local;                     // the waves may keep the exchange inside one XCD's L2 after checking their placement (xcc_announce, lstm_wave.hip)
  int wpb;                           // wave-autonomous forward: waves per block (1, 2 or 4)
  int no_stash;                      // forward only (evaluation): gates / cell states are not stashed
  short blk2role[MAXB];              // blockIdx -> linear role (-1: no role, exit at once); roles of one cluster share blockIdx % 8
};

// one per kernel file: the kernel of instance `id` (MMDA_LSTM_K_*) for the pass; nullptr: not this file's id, or not for this pass
typedef void (*Kernel)(CLaunch);
Kernel barrier_kernel(int id, bool bwd);
Kernel wave_kernel(int id, bool bwd);
Kernel quad_kernel(int id, bool bwd);

// xchg layout per descriptor: [0,64) abort word | flags: (dir, group, wg) x FLAG_STRIDE B | X: (dir, group, parity) x slot
// Flags: four 64-byte lines per workgroup.  The barrier-synchronised kernels signal on line 0; the wave-autonomous forward
// kernel signals per wave on line (m-tile * 2 + local hidden tile).
constexpr size_t FLAG_STRIDE = 256;
__host__ __device__ inline size_t xchg_flags_off() { return 64; }
__host__ __device__ inline size_t xchg_x_off(int ngroups_total, int NC) { return 64 + (size_t)2 * ngroups_total * NC * FLAG_STRIDE; }
// one exchange slot = one (direction, group, parity): forward uses GROUP x 4Hp bf16 of it, backward NC x GROUP x Hp
__host__ __device__ inline size_t xchg_slot(int NC, int Hp) {
  const size_t barrier_form = (size_t)(NC > 4 ? NC : 4) * GROUP * Hp * 2;
  // backward, wave-autonomous: [consumer tile][m-tile][producer tile (count rounded up to even)][64] x 8 B
  const size_t wave_form = (size_t)(Hp / 16) * 2 * (((Hp / 16) + 1) & ~1) * 512;
  return barrier_form > wave_form ? barrier_form : wave_form;
}
__host__ __device__ inline size_t xchg_bytes(int ngroups_total, int NC, int Hp) {
  return xchg_x_off(ngroups_total, NC) + (size_t)2 * ngroups_total * 2 * xchg_slot(NC, Hp);
}

__device__ __forceinline__ void st_flag(void* p, unsigned v) { __hip_atomic_store((gu32*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_flag_plain(void* p, unsigned v) { __hip_atomic_store((gu32*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ unsigned ld_flag(const void* p) { return __hip_atomic_load((gu32*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
// 16-byte write-through (sc1) store / L1-bypassing (sc1) load through a buffer descriptor built from wave-uniform values
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(void* p, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(p, 0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ void st16_sc1(__amdgpu_buffer_rsrc_t r, unsigned off, u32x4 v) { __builtin_amdgcn_raw_buffer_store_b128(v, r, off, 0, 16); }
__device__ __forceinline__ void st16_plain(__amdgpu_buffer_rsrc_t r, unsigned off, u32x4 v) { __builtin_amdgcn_raw_buffer_store_b128(v, r, off, 0, 0); }
__device__ __forceinline__ u32x4 ld16_sc1(__amdgpu_buffer_rsrc_t r, unsigned off) { return __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 16); }

struct Where { int di, dir, grp, me; };

// Branch-free global I/O: every per-step load/store goes through a buffer descriptor with a 32-bit byte offset; lanes
// that have nothing to do (padding columns, samples past the batch, t >= len_b) use an offset beyond the descriptor, for
// which the hardware returns 0 / drops the store.  (A load under a lane-dependent branch makes hipcc wait vmcnt(0) per
// element, and 64-bit index arithmetic per access costs ~20 VALU instructions.)
constexpr unsigned OOB = 0xFFFFFF00u;
__device__ __forceinline__ float ldf(__amdgpu_buffer_rsrc_t r, unsigned off) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, off, 0, 0));
}
// cache policy of the bulk stores -- stash, hseq, gate gradients: write-back.  (Measured at B=32, step in ms: write-back 0.722, nt
// 0.740, sc1 write-through 0.751, sc0 sc1 0.753: the end-of-kernel write-back of what is still dirty costs less than write-through
// traffic beside the hand-offs.)
constexpr int STASH_AUX = 0;
__device__ __forceinline__ void stf(__amdgpu_buffer_rsrc_t r, unsigned off, float v) {
  __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), r, off, 0, STASH_AUX);
}
__device__ __forceinline__ f32x4 ldf4(__amdgpu_buffer_rsrc_t r, unsigned off) {
  return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0));
}
__device__ __forceinline__ void stf4(__amdgpu_buffer_rsrc_t r, unsigned off, f32x4 v) {
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), r, off, 0, STASH_AUX);
}

// two floats -> one dword of two bf16 (round to nearest even): ONE v_cvt_pk_bf16_f32 on gfx950
__device__ __forceinline__ unsigned pack_bf16x2(float lo, float hi) {
  typedef float f32x2_t __attribute__((ext_vector_type(2)));
  typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
  return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2_t{lo, hi}, bf16x2_t));
}
constexpr unsigned FAR = 0x40000000u;      // added to a valid offset it lands beyond any exchange buffer (and does not wrap)
__device__ __forceinline__ unsigned my_xcc_id() { return __builtin_amdgcn_s_getreg(6164) & 15u; }           // HW_REG_XCC_ID[3:0]

}  // namespace mmda_resident
