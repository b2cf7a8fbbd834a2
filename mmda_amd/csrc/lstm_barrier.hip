// Resident recurrences, Barrier form (lstm_resident.h): a workgroup of four waves owns TPW <= 2 hidden tiles x the two m-tiles of a
// batch group, W_hh in LDS; the NC workgroups of a cluster (H = 300: 10) hand over with ONE flag each.  Some H > 320; LSTM only.
#include "lstm_resident.h"

namespace mmda_resident {
namespace {

__device__ __forceinline__ Where locate(const CLaunch& L, int role) {
  Where w;
  w.di = 0;
#pragma unroll
  for (int i = 1; i < MAXD; ++i)
    if (i < L.n && role >= L.d[i].wg_begin) w.di = i;
  const CDesc& D = L.d[w.di];
  int local = role - D.wg_begin;
  w.dir = local / (L.ng * D.NC);
  int rem = local % (L.ng * D.NC);
  w.grp = L.g0 + rem / D.NC;
  w.me = rem % D.NC;
  return w;
}

// Waits until every other workgroup of the cluster has published `epoch`.  Returns false (uniformly for the workgroup,
// through `lds_ok`) on timeout / abort.  Called by all threads.
__device__ __forceinline__ bool wait_cluster(unsigned char* flags, unsigned char* abort_w, int NC, int me, unsigned epoch,
                                             volatile int* lds_ok) {
  if ((threadIdx.x >> 6) == 0) {
    const int lane = threadIdx.x & 63;
    bool ok = true;
    if (lane < NC && lane != me) {
      unsigned spins = 0;
      while ((int)(ld_flag(flags + (size_t)lane * FLAG_STRIDE) - epoch) < 0) {
        ++spins;
        if (spins > SPIN_LIMIT || ((spins & 255u) == 0 && ld_flag(abort_w) != 0)) { ok = false; break; }
        __builtin_amdgcn_s_sleep(1);
      }
    }
    ok = __all(ok);
    if (lane == 0) {
      *lds_ok = ok ? 1 : 0;
      if (!ok) st_flag(abort_w, 1u);
    }
  }
  __syncthreads();
  return *lds_ok != 0;
}

// ------------------------------------------------------------------------------------------------ forward
// wave -> (m-tile mt = wave&1 : 16 of the group's 32 samples, local hidden tile lt = wave>>1 < TPW)
template <int KSC, bool GM>
__global__ __launch_bounds__(256, 1) void lstm_fwd_cluster_kernel(CLaunch L) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  // the serial chain of this kernel is the critical path of the step: its waves issue ahead of any GEMM waves that share the CU
  __builtin_amdgcn_s_setprio(3);
  const int role = L.blk2role[blockIdx.x];
  if (role < 0) return;
  const Where wh = locate(L, role);
  const CDesc& D = L.d[wh.di];
  const int H = D.H, Hp = D.Hp, Kp = D.Kp, KS = D.KS, nHT = D.nHT, TPW = D.TPW, NC = D.NC;
  const int B = L.B, T = L.T, dir = wh.dir, me = wh.me;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int mt = wave & 1, lt = wave >> 1;
  const int ht = me * TPW + lt;
  const bool tile_ok = lt < TPW && ht < nHT;             // wave-uniform
  const int col = ht * 16 + fr;
  const int ld = Kp + 8;
  const int XW = 4 * Hp;
  const int ngt = (B + GROUP - 1) / GROUP;
  const unsigned G4 = 4u * H;
  constexpr bool gm = GM;                               // layout of `gates` (compile time: both forms in one kernel cost registers)

  uint4* Wl = reinterpret_cast<uint4*>(smem);                                            // TPW*4*KS*64 x 16 B
  unsigned short* hb = reinterpret_cast<unsigned short*>(smem + (size_t)TPW * 4 * KS * 1024);   // 2 x GROUP x ld
  volatile int& lds_ok = *reinterpret_cast<volatile int*>(smem + (size_t)TPW * 4 * KS * 1024 + (size_t)2 * GROUP * ld * 2);

  unsigned char* abort_w = D.xchg;
  unsigned char* flags = D.xchg + xchg_flags_off() + ((size_t)(dir * ngt + wh.grp) * NC) * FLAG_STRIDE;
  unsigned char* Xb = D.xchg + xchg_x_off(ngt, NC) + ((size_t)(dir * ngt + wh.grp) * 2) * xchg_slot(NC, Hp);

  // resident weights: the forward packing is [(ht*4+g)*KS + ks][lane] x 16 B; this workgroup owns tiles me*TPW..+TPW
  {
    const uint4* src = reinterpret_cast<const uint4*>(D.wpack[dir]);
    const int per_tile = 4 * KS * 64;
    if (!(KSC > 0 && KS == KSC))                          // register-resident weights need no LDS copy
    for (int i = tid; i < TPW * per_tile; i += 256) {
      int l2 = i / per_tile, h2 = me * TPW + l2;
      Wl[i] = h2 < nHT ? src[(size_t)h2 * per_tile + (i % per_tile)] : uint4{0, 0, 0, 0};
    }
    for (int i = tid; i < 2 * GROUP * ld; i += 256) hb[i] = 0;
  }
  const __amdgpu_buffer_rsrc_t rg = make_rsrc(D.gates, (unsigned)T * B * 2u * G4 * 4u);
  // cell-state stash: (T,B,2,H) fp32; with the gate-minor layout it is batch-minor-by-4, (T, ceil(B/4), 2, H, 4): the four samples a
  // lane owns are 16 contiguous bytes (one access in the wave-autonomous kernels instead of four)
  const __amdgpu_buffer_rsrc_t rc = make_rsrc(D.cstash, (unsigned)T * (GM ? (unsigned)((B + 3) & ~3) : (unsigned)B) * 2u * H * 4u);
  const unsigned scc = GM ? (unsigned)((B + 3) >> 2) * 2u * H * 16u : (unsigned)B * 2u * H * 4u;      // its byte stride per time step
  const __amdgpu_buffer_rsrc_t rh = make_rsrc(D.hseq, (unsigned)T * B * 2u * H * 4u);
  const unsigned sg = (unsigned)B * 2u * G4 * 4u, sc = (unsigned)B * 2u * H * 4u;   // byte strides per time step (hseq: sc too)
  unsigned og[4], oc[4], oh[4];
  int len_r[4];
  bool inb[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int b = wh.grp * GROUP + mt * 16 + fq * 4 + r;
    inb[r] = tile_ok && col < H && b < B;
    const int lv = L.lengths[min(b, B - 1)];
    len_r[r] = inb[r] ? lv : 0;
    og[r] = (((unsigned)b * 2u + dir) * G4 + (gm ? col * 4 : col)) * 4u;
    oc[r] = GM ? ((((((unsigned)b >> 2) * 2u + dir) * H + col) << 2) + ((unsigned)b & 3u)) * 4u : (((unsigned)b * 2u + dir) * H + col) * 4u;
    oh[r] = ((unsigned)b * 2u * H + dir * H + col) * 4u;
  }
  float c_reg[4] = {0.f, 0.f, 0.f, 0.f}, h_reg[4] = {0.f, 0.f, 0.f, 0.f};
  float pre[2][4][4];                                   // input-to-hidden pre-activations, prefetched TWO steps ahead
  // register-resident W_hh fragments of this wave's hidden tile (compile-time KS only; see do_step)
  bf16x8 wreg[4][KSC > 0 ? KSC : 1];
  if (KSC > 0 && KS == KSC) {
    const bf16x8* src = reinterpret_cast<const bf16x8*>(D.wpack[dir]);
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int k2 = 0; k2 < (KSC > 0 ? KSC : 1); ++k2)
        wreg[g][k2] = tile_ok ? src[((size_t)(ht * 4 + g) * KSC + k2) * 64 + lane] : bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
  }

  auto load_pre = [&](float (&dst)[4][4], int step) {
    const int t = dir ? T - 1 - step : step;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool act = step < T && t < len_r[r];
      const unsigned o = og[r] + (unsigned)t * sg;
      if (gm) {
        const f32x4 v = ldf4(rg, act ? o : OOB);
#pragma unroll
        for (int g = 0; g < 4; ++g) dst[g][r] = v[g];
      } else {
#pragma unroll
        for (int g = 0; g < 4; ++g) dst[g][r] = ldf(rg, act ? o + g * H * 4u : OOB);
      }
    }
  };
  load_pre(pre[0], 0);
  load_pre(pre[1], 1);
  if (tid == 0) lds_ok = 1;
  __syncthreads();
  __amdgpu_buffer_rsrc_t xr[2];
  xr[0] = make_rsrc(Xb, (unsigned)(GROUP * XW * 2));
  xr[1] = make_rsrc(Xb + xchg_slot(NC, Hp), (unsigned)(GROUP * XW * 2));

  // all-gather tables (fixed for the whole sequence): X byte offset (OOB = nothing to fetch) and LDS destination
  unsigned goff[8]; int gdst0[8];
  {
    const int cprow = Hp / 8;                            // 16-byte chunks per row over all hidden tiles
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      int i = u * 256 + tid;
      int row = i / cprow, cc = (i % cprow) * 8;
      bool want = i < GROUP * cprow && cc / (TPW * 16) != me;
      gdst0[u] = want ? row * ld + cc : -1;
      goff[u] = want ? (unsigned)((row * XW + cc) * 2) : OOB;
    }
  }
  unsigned long long ph[8] = {0, 0, 0, 0, 0, 0, 0, 0}, last = 0;
#define STAMP(i) do { if (L.dbg && tid == 0) { unsigned long long now_ = __builtin_readcyclecounter(); ph[i] += now_ - last; last = now_; } } while (0)
  if (L.dbg && tid == 0) last = __builtin_readcyclecounter();

  auto store_stash = [&](const float (&sv)[4][6], int t) {
    if (!tile_ok) return;                                // wave-uniform
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool act = t < len_r[r];
      const unsigned o = act ? og[r] + (unsigned)t * sg : OOB;
      if (gm) {
        stf4(rg, o, f32x4{sv[r][0], sv[r][1], sv[r][2], sv[r][3]});
      } else {
        stf(rg, o, sv[r][0]); stf(rg, act ? o + H * 4u : OOB, sv[r][1]); stf(rg, act ? o + 2u * H * 4u : OOB, sv[r][2]);
        stf(rg, act ? o + 3u * H * 4u : OOB, sv[r][3]);
      }
      stf(rc, act ? oc[r] + (unsigned)t * scc : OOB, sv[r][4]);
      stf(rh, inb[r] ? oh[r] + (unsigned)t * sc : OOB, sv[r][5]);     // zero at padded positions (pad_packed_sequence)
    }
  };
  // one time step with the pre-activation buffer `P` (static index: the loop below is unrolled by two)
  auto do_step = [&](int step, float (&P)[4][4], int cur) -> bool {
    const int t = dir ? T - 1 - step : step;
    const unsigned epoch = L.epoch_base + (unsigned)step + 1u;
    float sv[4][6];
    if (tile_ok) {
      f32x4 acc[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
      const unsigned short* hrow = hb + (cur * GROUP + mt * 16 + fr) * ld + fq * 8;
      const bf16x8* wp = reinterpret_cast<const bf16x8*>(Wl) + (size_t)(lt * 4) * KS * 64 + lane;
      if (KSC > 0 && KS == KSC) {
        // compile-time trip count (text: 10): the 40 W_hh fragments of this wave's hidden tile live in REGISTERS for the whole
        // sequence (wreg, 160 VGPRs; the kernel runs one wave per SIMD, so 512 are available).  Per step only the ten h
        // fragments come from LDS; re-reading the weights from LDS cost 200 KB of LDS traffic per step and workgroup, which
        // at 128 B/clk was longer than the MFMAs themselves.
        bf16x8 af[KSC];
#pragma unroll
        for (int k2 = 0; k2 < KSC; ++k2) af[k2] = *reinterpret_cast<const bf16x8*>(hrow + k2 * 32);
        __builtin_amdgcn_sched_barrier(0);           // all ten reads in flight before the first MFMA (else hipcc serialises read -> wait -> 4 MFMAs)
#pragma unroll
        for (int k2 = 0; k2 < KSC; ++k2) {
#pragma unroll
          for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[k2], wreg[g][k2], acc[g], 0, 0, 0);
        }
      } else {
#pragma unroll 2
        for (int ks = 0; ks < KS; ++ks) {
          bf16x8 a = *reinterpret_cast<const bf16x8*>(hrow + ks * 32);
#pragma unroll
          for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, wp[(g * KS + ks) * 64], acc[g], 0, 0, 0);
        }
      }
      if (L.dbg) { asm volatile("s_nop 0" :: "v"(acc[0][0]), "v"(acc[1][0]), "v"(acc[2][0]), "v"(acc[3][0])); STAMP(7); }
      // lane-local cell update, branch-free (inactive lanes compute on zeros and are masked by the selects / OOB stores)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool act = t < len_r[r];
        const float gi = sigmoid_fast(acc[0][r] + P[0][r]);
        const float gf = sigmoid_fast(acc[1][r] + P[1][r]);
        const float gg = tanh_fast(acc[2][r] + P[2][r]);
        const float go = sigmoid_fast(acc[3][r] + P[3][r]);
        const float cn = gf * c_reg[r] + gi * gg;
        const float hn = go * tanh_fast(cn);
        c_reg[r] = act ? cn : c_reg[r];
        h_reg[r] = act ? hn : h_reg[r];
        hb[((cur ^ 1) * GROUP + mt * 16 + fq * 4 + r) * ld + col] = f2bf(h_reg[r]);
        sv[r][0] = gi; sv[r][1] = gf; sv[r][2] = gg; sv[r][3] = go; sv[r][4] = cn; sv[r][5] = act ? hn : 0.f;
      }
      // stash for the backward pass.  Measured: issued here (the publish drain covers it) beats issuing it after the flag store
      // (the polling wave's flag reads queue behind it) or behind the gather loads (its ~40 VMEM issues then sit on the chain).
      store_stash(sv, t);
    }
    STAMP(0);
    __syncthreads();                                     // own h slice complete in LDS
    STAMP(1);
    bool ok = true;
    if (NC > 1) {
      __amdgpu_buffer_rsrc_t X = (epoch & 1u) ? xr[1] : xr[0];
      const int cpr = TPW * 2;                           // 16-byte chunks of the own slice per row
      const int c0 = me * TPW * 16;
      for (int i = tid; i < GROUP * cpr; i += 256) {
        int row = i / cpr, cc = c0 + (i % cpr) * 8;
        if (cc >= Hp) continue;                          // last workgroup: tiles past the padded width do not exist
        u32x4 v = *reinterpret_cast<const u32x4*>(&hb[((cur ^ 1) * GROUP + row) * ld + cc]);
        if (L.xcd_local) st16_plain(X, (unsigned)((row * XW + cc) * 2), v);
        else st16_sc1(X, (unsigned)((row * XW + cc) * 2), v);
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every storing wave drains its write-through stores
      STAMP(2);
      __syncthreads();
      if (tid == 0) { if (L.xcd_local) st_flag_plain(flags + (size_t)me * FLAG_STRIDE, epoch); else st_flag(flags + (size_t)me * FLAG_STRIDE, epoch); }
      STAMP(3);
      load_pre(P, step + 2);                             // lands while the cluster is being polled
      ok = wait_cluster(flags, abort_w, NC, me, epoch, &lds_ok);
      STAMP(4);
      if (ok) {
        u32x4 gv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) gv[u] = ld16_sc1(X, goff[u]);
        STAMP(5);
        const int nb = (cur ^ 1) * GROUP * ld;
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (gdst0[u] >= 0) *reinterpret_cast<u32x4*>(&hb[nb + gdst0[u]]) = gv[u];
      }
    } else {
      load_pre(P, step + 2);
    }
    STAMP(6);
    __syncthreads();
    STAMP(7);
    return ok;
  };
  {
    int step = 0, cur = 0;
    for (; step + 1 < T; step += 2) {
      if (!do_step(step, pre[0], cur)) { step = T; break; }
      if (!do_step(step + 1, pre[1], cur ^ 1)) { step = T; break; }
    }
    if (step < T) do_step(step, pre[0], cur);
  }
  if (L.dbg && tid == 0) {
    for (int i = 0; i < 8; ++i) L.dbg[(size_t)role * 8 + i] = ph[i];
    if (L.xcd_local < 0) L.dbg[(size_t)role * 8 + 7] = ((unsigned long long)blockIdx.x << 32) | (unsigned)__builtin_amdgcn_s_getreg(6164);   // XCC_ID
  }
#undef STAMP
  // final hidden state straight into the utterance layout [h1_fwd, h2_fwd, h1_bwd, h2_bwd] (models.py:203)
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int b = wh.grp * GROUP + mt * 16 + fq * 4 + r;
    if (inb[r]) D.utt[(int64_t)b * 4 * H + (dir * 2 + D.layer) * H + col] = h_reg[r];
  }
}

// ------------------------------------------------------------------------------------------------ backward
// dh_{t-1} = dG_t W_hh.  The workgroup owns the GATE ROWS of its hidden units (K = TPW*64 rows of W_hh, all Hp columns,
// resident in LDS) and computes a PARTIAL dh over all hidden columns from its own dG slice; the partials are then
// reduce-scattered inside the cluster: each workgroup publishes its (GROUP x Hp) bf16 partial and gathers only the
// 2*TPW*16-byte column slices of its own units from the other NC-1 workgroups (18 KB per step for the text LSTM instead of
// the 70 KB an all-gather of dG would cost), sums them in fp32 and continues with its lane-local cell backward.
constexpr int MAXNT = 16;          // n-tiles per wave (two waves share an m-tile): supports nHT <= 32
constexpr int BPU = 8, BGU = 8;    // publish / gather 16-byte chunks per thread (text: 5 and 5)

template <bool GM>
__global__ __launch_bounds__(256, 1) void lstm_bwd_cluster_kernel(CLaunch L) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  // the serial chain of this kernel is the critical path of the step: its waves issue ahead of any GEMM waves that share the CU
  __builtin_amdgcn_s_setprio(3);
  const int role = L.blk2role[blockIdx.x];
  if (role < 0) return;
  const Where wh = locate(L, role);
  const CDesc& D = L.d[wh.di];
  const int H = D.H, Hp = D.Hp, nHT = D.nHT, TPW = D.TPW, NC = D.NC;
  const int B = L.B, T = L.T, dir = wh.dir, me = wh.me;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int mt = wave & 1, lt = wave >> 1;
  const int ht = me * TPW + lt;
  const bool tile_ok = lt < TPW && ht < nHT;
  const int col = ht * 16 + fr;
  const int KW = TPW * 64, lda = KW + 8, lds = Hp + 8, OW = TPW * 16;
  const int ngt = (B + GROUP - 1) / GROUP;
  const unsigned G4 = 4u * H;
  constexpr bool gm = GM;                               // layout of `gates` (compile time: both forms in one kernel cost registers)

  // LDS: W slice [lt][nt][ks2] fragments | A (own dG) | staging (partial dh) | gathered partials | flag
  size_t off = 0;
  uint4* Wl = reinterpret_cast<uint4*>(smem);                        off += (size_t)TPW * nHT * 2 * 1024;
  unsigned short* Ab = reinterpret_cast<unsigned short*>(smem + off); off += (size_t)GROUP * lda * 2;
  unsigned short* St = reinterpret_cast<unsigned short*>(smem + off); off += (size_t)GROUP * lds * 2;
  unsigned short* Gb = reinterpret_cast<unsigned short*>(smem + off); off += (size_t)(NC > 1 ? NC - 1 : 1) * GROUP * OW * 2;
  volatile int& lds_ok = *reinterpret_cast<volatile int*>(smem + off);

  unsigned char* abort_w = D.xchg;
  unsigned char* flags = D.xchg + xchg_flags_off() + ((size_t)(dir * ngt + wh.grp) * NC) * FLAG_STRIDE;
  unsigned char* Xb = D.xchg + xchg_x_off(ngt, NC) + ((size_t)(dir * ngt + wh.grp) * 2) * xchg_slot(NC, Hp);
  {
    // cluster-backward packing: [(ht*nHT + nt)*2 + ks2][lane] x 16 B; the tiles of this workgroup are contiguous blocks
    const uint4* src = reinterpret_cast<const uint4*>(D.wpack_c[dir]);
    const int per_tile = nHT * 2 * 64;
    for (int i = tid; i < TPW * per_tile; i += 256) {
      int l2 = i / per_tile, h2 = me * TPW + l2;
      Wl[i] = h2 < nHT ? src[(size_t)h2 * per_tile + (i % per_tile)] : uint4{0, 0, 0, 0};
    }
    for (int i = tid; i < GROUP * lda; i += 256) Ab[i] = 0;
    for (int i = tid; i < GROUP * lds; i += 256) St[i] = 0;
    for (int i = tid; i < (NC > 1 ? NC - 1 : 1) * GROUP * OW; i += 256) Gb[i] = 0;
  }
  const __amdgpu_buffer_rsrc_t rg = make_rsrc(D.gates, (unsigned)T * B * 2u * G4 * 4u);
  // cell-state stash: (T,B,2,H) fp32; with the gate-minor layout it is batch-minor-by-4, (T, ceil(B/4), 2, H, 4): the four samples a
  // lane owns are 16 contiguous bytes (one access in the wave-autonomous kernels instead of four)
  const __amdgpu_buffer_rsrc_t rc = make_rsrc(D.cstash, (unsigned)T * (GM ? (unsigned)((B + 3) & ~3) : (unsigned)B) * 2u * H * 4u);
  const unsigned scc = GM ? (unsigned)((B + 3) >> 2) * 2u * H * 16u : (unsigned)B * 2u * H * 4u;      // its byte stride per time step
  const __amdgpu_buffer_rsrc_t rd = make_rsrc(const_cast<float*>(D.d_hseq), D.d_hseq ? (unsigned)T * B * 2u * H * 4u : 0u);
  const __amdgpu_buffer_rsrc_t ru = make_rsrc(D.utt, (unsigned)B * 4u * H * 4u);
  const unsigned sg = (unsigned)B * 2u * G4 * 4u, sc = (unsigned)B * 2u * H * 4u;
  unsigned og[4], oc[4], oh[4];
  int len_r[4];
  bool inb[4];
  float d_fin[4];                                       // gradient of the final hidden state of this (sample, unit)
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int b = wh.grp * GROUP + mt * 16 + fq * 4 + r;
    inb[r] = tile_ok && col < H && b < B;
    const int lv = L.lengths[min(b, B - 1)];
    len_r[r] = inb[r] ? lv : 0;
    og[r] = (((unsigned)b * 2u + dir) * G4 + (gm ? col * 4 : col)) * 4u;
    oc[r] = GM ? ((((((unsigned)b >> 2) * 2u + dir) * H + col) << 2) + ((unsigned)b & 3u)) * 4u : (((unsigned)b * 2u + dir) * H + col) * 4u;
    oh[r] = ((unsigned)b * 2u * H + dir * H + col) * 4u;
    d_fin[r] = ldf(ru, inb[r] ? ((unsigned)b * 4u * H + (dir * 2 + D.layer) * H + col) * 4u : OOB);
  }
  float dh_rec[4] = {0.f, 0.f, 0.f, 0.f}, dc[4] = {0.f, 0.f, 0.f, 0.f};
  struct Stash { float g[4][4], c[4], cp[4], dh[4]; };
  Stash sb[2];                                          // forward stash of the coming steps, prefetched TWO steps ahead

  auto load_stash = [&](Stash& S, int step) {
    const int t = dir ? step : T - 1 - step;
    const int tp = dir ? t + 1 : t - 1;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool act = step < T && t < len_r[r];
      const unsigned o = og[r] + (unsigned)t * sg;
      if (gm) {
        const f32x4 v = ldf4(rg, act ? o : OOB);
#pragma unroll
        for (int g = 0; g < 4; ++g) S.g[g][r] = v[g];
      } else {
#pragma unroll
        for (int g = 0; g < 4; ++g) S.g[g][r] = ldf(rg, act ? o + g * H * 4u : OOB);
      }
      S.c[r] = ldf(rc, act ? oc[r] + (unsigned)t * scc : OOB);
      S.cp[r] = ldf(rc, (act && tp >= 0 && tp < len_r[r]) ? oc[r] + (unsigned)tp * scc : OOB);
      S.dh[r] = ldf(rd, act ? oh[r] + (unsigned)t * sc : OOB);          // zero-record descriptor when d_hseq == NULL
    }
  };
  load_stash(sb[0], 0);
  load_stash(sb[1], 1);
  if (tid == 0) lds_ok = 1;
  __amdgpu_buffer_rsrc_t xr[2];
  xr[0] = make_rsrc(Xb, (unsigned)(NC * GROUP * Hp * 2));
  xr[1] = make_rsrc(Xb + xchg_slot(NC, Hp), (unsigned)(NC * GROUP * Hp * 2));
  // publish table: 16-byte chunks of the staged partial that belong to OTHER workgroups' columns -> X[me][row][col]
  unsigned poff[BPU]; int psrc[BPU];
  // gather table: the own-column chunks of every other workgroup's partial -> Gb[src'][row][.]
  unsigned goff[BGU]; int gdst[BGU];
  {
    const int cprow = Hp / 8, cpo = OW / 8;
    const int own_lo = me * OW, own_hi = own_lo + OW;
#pragma unroll
    for (int u = 0; u < BPU; ++u) {
      int i = u * 256 + tid;
      int row = i / cprow, cc = (i % cprow) * 8;
      bool want = NC > 1 && i < GROUP * cprow && !(cc >= own_lo && cc < own_hi);
      psrc[u] = want ? row * lds + cc : 0;
      poff[u] = want ? (unsigned)(((me * GROUP + row) * Hp + cc) * 2) : OOB;
    }
#pragma unroll
    for (int u = 0; u < BGU; ++u) {
      int i = u * 256 + tid;
      int sp = i / (GROUP * cpo), rem = i % (GROUP * cpo);
      int row = rem / cpo, ch = rem % cpo;
      int src = sp < me ? sp : sp + 1;
      bool want = NC > 1 && sp < NC - 1 && own_lo + ch * 8 < Hp;
      gdst[u] = want ? (sp * GROUP + row) * OW + ch * 8 : -1;
      goff[u] = want ? (unsigned)(((src * GROUP + row) * Hp + own_lo + ch * 8) * 2) : OOB;
    }
  }
  __syncthreads();

  auto do_step = [&](int step, Stash& S) -> bool {
    const int t = dir ? step : T - 1 - step;
    const unsigned epoch = L.epoch_base + (unsigned)step + 1u;
    // (1) lane-local gate gradients of the own hidden units (branch-free); A operand into LDS, fp32 dG in place over the stash
    float dgv[4][4];
    auto store_dg = [&]() {
      if (!tile_ok) return;                              // wave-uniform
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const unsigned o = inb[r] ? og[r] + (unsigned)t * sg : OOB;       // zero at padded positions too
        if (gm) {
          stf4(rg, o, f32x4{dgv[r][0], dgv[r][1], dgv[r][2], dgv[r][3]});
        } else {
#pragma unroll
          for (int g = 0; g < 4; ++g) stf(rg, inb[r] ? o + g * H * 4u : OOB, dgv[r][g]);
        }
      }
    };
    if (tile_ok) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool act = t < len_r[r];
        const bool fin = dir ? (t == 0) : (t == len_r[r] - 1);
        const float gi = S.g[0][r], gf = S.g[1][r], gg = S.g[2][r], go = S.g[3][r];
        const float dh = dh_rec[r] + S.dh[r] + (fin ? d_fin[r] : 0.f);
        const float tc = tanh_fast(S.c[r]);
        const float dct = dc[r] + dh * go * (1.f - tc * tc);
        float dp[4];
        dp[0] = act ? dct * gg * gi * (1.f - gi) : 0.f;
        dp[1] = act ? dct * S.cp[r] * gf * (1.f - gf) : 0.f;
        dp[2] = act ? dct * gi * (1.f - gg * gg) : 0.f;
        dp[3] = act ? dh * tc * go * (1.f - go) : 0.f;
        dc[r] = act ? dct * gf : dc[r];
        const int row = mt * 16 + fq * 4 + r;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          Ab[row * lda + lt * 64 + g * 16 + fr] = f2bf(dp[g]);
          dgv[r][g] = dp[g];                             // fp32 dG goes to memory after the publish (off the chain)
        }
      }
    }
    __syncthreads();                                     // own dG slice (A operand) complete
    // (2) partial dh over ALL hidden columns: (16 x KW) x (KW x 16) per n-tile, W_hh rows of the own units from LDS
    {
      bf16x8 af[4];
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
        af[ks] = *reinterpret_cast<const bf16x8*>(&Ab[(mt * 16 + fr) * lda + (ks < TPW * 2 ? ks : 0) * 32 + fq * 8]);
      const bf16x8* wbase = reinterpret_cast<const bf16x8*>(Wl) + lane;
#pragma unroll
      for (int i = 0; i < MAXNT; ++i) {
        const int nt = (wave >> 1) + 2 * i;
        if (nt >= nHT) break;
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
          if (ks < TPW * 2) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[ks], wbase[(((ks >> 1) * nHT + nt) * 2 + (ks & 1)) * 64], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) St[(mt * 16 + fq * 4 + r) * lds + nt * 16 + fr] = f2bf(acc[r]);
      }
    }
    __syncthreads();                                     // staged partial complete
    bool ok = true;
    if (NC > 1) {
      __amdgpu_buffer_rsrc_t X = (epoch & 1u) ? xr[1] : xr[0];
#pragma unroll
      for (int u = 0; u < BPU; ++u) {
        u32x4 v = *reinterpret_cast<const u32x4*>(&St[psrc[u]]);
        if (L.xcd_local) st16_plain(X, poff[u], v);
        else st16_sc1(X, poff[u], v);                    // out-of-range offsets (own columns / past the end) are dropped
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if (tid == 0) { if (L.xcd_local) st_flag_plain(flags + (size_t)me * FLAG_STRIDE, epoch); else st_flag(flags + (size_t)me * FLAG_STRIDE, epoch); }
      store_dg();                                        // off the chain: the drain above only waited for the publish stores
      load_stash(S, step + 2);                           // lands while the cluster is being polled
      ok = wait_cluster(flags, abort_w, NC, me, epoch, &lds_ok);
      if (ok) {
        u32x4 gv[BGU];
#pragma unroll
        for (int u = 0; u < BGU; ++u) gv[u] = ld16_sc1(X, goff[u]);
#pragma unroll
        for (int u = 0; u < BGU; ++u)
          if (gdst[u] >= 0) *reinterpret_cast<u32x4*>(&Gb[gdst[u]]) = gv[u];
      }
      __syncthreads();
    } else {
      store_dg();
      load_stash(S, step + 2);
    }
    // (3) reduce: dh_{t-1} of the own units = own partial + the NC-1 gathered partials (fp32 sum of bf16 partials)
    if (tile_ok) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = mt * 16 + fq * 4 + r;
        float sum = bf2f(St[row * lds + me * OW + lt * 16 + fr]);
        for (int sp = 0; sp < NC - 1; ++sp) sum += bf2f(Gb[(sp * GROUP + row) * OW + lt * 16 + fr]);
        dh_rec[r] = sum;
      }
    }
    return ok;
  };
  {
    int step = 0;
    for (; step + 1 < T; step += 2) {
      if (!do_step(step, sb[0])) { step = T; break; }
      if (!do_step(step + 1, sb[1])) { step = T; break; }
    }
    if (step < T) do_step(step, sb[0]);
  }
}

}  // namespace

Kernel barrier_kernel(int id, bool bwd) {
  Kernel f = nullptr, b = nullptr;
  switch (id) {
    case MMDA_LSTM_K_FWD_BARRIER_GM: f = lstm_fwd_cluster_kernel<10, true>; break;
    case MMDA_LSTM_K_FWD_BARRIER: f = lstm_fwd_cluster_kernel<10, false>; break;
    case MMDA_LSTM_K_BWD_BARRIER_GM: b = lstm_bwd_cluster_kernel<true>; break;
    case MMDA_LSTM_K_BWD_BARRIER: b = lstm_bwd_cluster_kernel<false>; break;
  }
  return bwd ? b : f;
}

}  // namespace mmda_resident
