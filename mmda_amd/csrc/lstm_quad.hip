// Resident recurrences, Quad form (lstm_resident.h): a workgroup of four waves owns one (m-tile, hidden tile) and splits the step's
// serial work four ways; after the first steps the hand-over needs no flags, the published data carry an epoch tag.  Runs when every
// descriptor has H <= 320, the layout is gate-minor and every tile of every batch group fits one launch; LSTM and GRU cells.
#include "lstm_resident.h"
#include <type_traits>

namespace mmda_resident {
namespace {

// ------------------------------------------------------------------------------------------------ forward, four waves per tile
// The wave-autonomous kernel (lstm_wave.hip) spends its step inside ONE wave: 40 MFMAs (~640 cycles), 40 quarter-rate transcendentals plus the
// cell arithmetic for 16 elements per lane (~1200 cycles), 24 memory instructions.  Here a (16-sample m-tile, 16-unit hidden tile)
// belongs to a WORKGROUP of four waves that split the step's serial work four ways:
//   k-split  wave w multiplies k-steps w, w+4, w+8 of h_{t-1} W_hh^T for all four gates (<= 12 MFMAs); it polls the flags of -- and
//            loads fragments from -- the <= 6 hidden tiles those k-steps cover, nothing else
//   reduce   the four partial 16 x 64 gate tiles meet in LDS (one 16-byte write per accumulator row, ONE workgroup barrier per step,
//            double buffered by step parity), summed in a fixed order (wave 0..3)
//   cell     wave w then owns samples 4w..4w+3 of the tile: ONE element per lane (5 exp + 5 rcp instead of 20 + 20), one 16-byte
//            stash store, one cell-state and one h store per lane
//   publish  the wave's four rows of the tile are 128 contiguous bytes of the exchange image (one line): one 2-byte store per lane,
//            drained, then the wave raises ITS flag (dword w of the tile's flag line, bytes 32..47; the placement announcement sits at
//            bytes 48..55 -- the wave-autonomous kernels use bytes 0..15 of the same lines)
// A publish at step s+2 overwrites the image of step s: it happens after the workgroup barrier of step s+2, i.e. after the four
// waves together have seen every tile's four flags for step s+1, hence after every reader of the step-s image has finished with it.
// A wave whose poll times out raises the abort word and from then on stops waiting (its results are garbage, the host discards the
// launch) but keeps arriving at the barriers, so the grid always drains.
// Steady-state data polling: one copy of a wave's three loads in flight, issued at once.  Measured at B=32 (step, ms): one copy 0.740
// (0 / 256 / 512 cycles of first delay: equal, 1024: 0.763), two copies issued back to back 0.738, two spaced by 512 / 1024 cycles
// 0.92 / 0.90, three 1.03, four 1.15 -- every read in flight sits in the consumer CU's memory queue in front of the one that will
// return the data, so polling harder makes the hand-off slower.
// ... and POLL_SLEEP x 64 cycles of s_sleep between a stale answer and the next question (B=32 step 0.676 -> 0.668 ms; 128 / 256
// cycles: 0.676 / 0.692)
constexpr int POLL_SLEEP = 1;

__device__ __forceinline__ bool flags4_reached(u32x4 f, unsigned need) {
  return (int)(f[0] - need) >= 0 && (int)(f[1] - need) >= 0 && (int)(f[2] - need) >= 0 && (int)(f[3] - need) >= 0;
}
// lane-per-tile poll of the four wave flags of a tile (one 16-byte L1-bypassing load); three reads in flight (see poll_tiles)
__device__ __forceinline__ bool poll_tiles4(__amdgpu_buffer_rsrc_t fr4, unsigned off, const unsigned char* abort_w, bool watching, unsigned need) {
  u32x4 f0 = ld16_sc1(fr4, off);
  __builtin_amdgcn_s_sleep(2);
  u32x4 f1 = ld16_sc1(fr4, off);
  __builtin_amdgcn_s_sleep(2);
  u32x4 f2 = ld16_sc1(fr4, off);
  for (unsigned spins = 0;; spins += 3) {
    if (__all(!watching || flags4_reached(f0, need))) return true;
    f0 = ld16_sc1(fr4, off);
    if (__all(!watching || flags4_reached(f1, need))) return true;
    f1 = ld16_sc1(fr4, off);
    if (__all(!watching || flags4_reached(f2, need))) return true;
    f2 = ld16_sc1(fr4, off);
    if (spins > SPIN_LIMIT || ((spins & 255u) == 0 && spins && ld_flag(abort_w) != 0)) return false;
  }
}

template <int CELL, int NST>
__global__ __launch_bounds__(256, 4) void lstm_fwd_quad_kernel(CLaunch L) {   // (<= 128 registers: four workgroups share a CU at large batches)
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __builtin_amdgcn_s_setprio(3);
  const int role = L.blk2role[blockIdx.x];
  if (role < 0) return;
  Where wh;
  wh.di = 0;
#pragma unroll
  for (int i = 1; i < MAXD; ++i)
    if (i < L.n && role >= L.d[i].wg_begin) wh.di = i;
  const CDesc& D = L.d[wh.di];
  {
    const int local = role - D.wg_begin;
    wh.dir = local / (L.ng * D.NCw);
    const int rem = local % (L.ng * D.NCw);
    wh.grp = L.g0 + rem / D.NCw;
    wh.me = rem % D.NCw;
  }
  const int H = D.H, Hp = D.Hp, KS = D.KS, nHT = D.nHT, NC = D.NC;
  const int B = L.B, T = L.T, dir = wh.dir;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int fr = lane & 15, fq = lane >> 4;             // MFMA frame: operand row / accumulator column fr, accumulator rows 4 fq ..+3
  const int rho = wh.me;                                // one workgroup per (hidden tile, m-tile)
  const int mt = rho & 1, ht = rho >> 1;
  const int row = 4 * w + fq, b = wh.grp * GROUP + mt * 16 + row, col = ht * 16 + fr;      // cell frame: the lane's one element
  const int ngt = (B + GROUP - 1) / GROUP;
  const unsigned G4 = 4u * H;
  float* red = reinterpret_cast<float*>(smem);

  unsigned char* abort_w = D.xchg;
  unsigned char* flags = D.xchg + xchg_flags_off() + ((size_t)(dir * ngt + wh.grp) * NC) * FLAG_STRIDE;
  unsigned char* Xb = D.xchg + xchg_x_off(ngt, NC) + ((size_t)(dir * ngt + wh.grp) * 2) * xchg_slot(NC, Hp);
  unsigned char* my_line = flags + (size_t)rho * 64;
  unsigned char* my_flag = my_line + 32 + 4 * w;
  const __amdgpu_buffer_rsrc_t fr4 = make_rsrc(flags, (unsigned)(2 * nHT) * 64u);
  // steps 1 and 2 (flags): lane tau watches the four wave flags of tile tau
  const bool awatch = lane < nHT;
  const unsigned aoff = awatch ? (unsigned)(lane * 2 + mt) * 64u + 32u : OOB;

  bf16x8 wreg[4][3];
  {
    const bf16x8* src = reinterpret_cast<const bf16x8*>(D.wpack[dir]);
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const int k2 = w + 4 * j;
        wreg[g][j] = k2 < KS ? src[((size_t)(ht * 4 + g) * KS + k2) * 64 + lane] : bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
      }
  }
  const __amdgpu_buffer_rsrc_t rg = make_rsrc(D.gates, (unsigned)T * B * 2u * G4 * 4u);
  const __amdgpu_buffer_rsrc_t rc = make_rsrc(D.cstash, (unsigned)T * (unsigned)((B + 3) & ~3) * 2u * H * 4u);
  const unsigned scc = (unsigned)((B + 3) >> 2) * 2u * H * 16u;
  const __amdgpu_buffer_rsrc_t rh = make_rsrc(D.hseq, (unsigned)T * B * 2u * H * 4u);
  const unsigned sg = (unsigned)B * 2u * G4 * 4u, sc = (unsigned)B * 2u * H * 4u;
  const bool inb = col < H && b < B;
  const int len = inb ? L.lengths[min(b, B - 1)] : 0;
  const unsigned og = (((unsigned)b * 2u + dir) * G4 + col * 4) * 4u;
  const unsigned oc = ((((((unsigned)b >> 2) * 2u + dir) * H + col) << 2) + ((unsigned)b & 3u)) * 4u;
  const unsigned oh = ((unsigned)b * 2u * H + dir * H + col) * 4u;
  float c_reg = 0.f, h_reg = 0.f;
  f32x4 pre[2];
  auto load_pre = [&](f32x4& dst, int step) {
    const int t = dir ? T - 1 - step : step;
    dst = ldf4(rg, (step < T && t < len) ? og + (unsigned)t * sg : OOB);
  };
  load_pre(pre[0], 0);
  load_pre(pre[1], 1);
  const unsigned slot_b = (unsigned)xchg_slot(NC, Hp);
  const unsigned img_b = (unsigned)nHT * 2u * 512u;
  const __amdgpu_buffer_rsrc_t xr = make_rsrc(Xb, slot_b + img_b);
  // A fragment of k-step k2: tile 2 k2 + (fq >> 1), row fr, units 8 (fq & 1) ..+7 (the tile-major image of the wave-autonomous form)
  unsigned foff[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int k2 = w + 4 * j;
    foff[j] = (k2 < KS && 2 * k2 + (fq >> 1) < nHT) ? (unsigned)(((((fq >> 1) * 2 + mt) * 256) + fr * 16 + 8 * (fq & 1)) * 2) + (unsigned)k2 * 2048u : FAR;
  }
  const unsigned pub_off = (unsigned)((((ht * 2 + mt) * 256) + row * 16 + fr) * 2);
  constexpr unsigned TAGS = 0x40004000u;                // bit 14 of both bf16 halves of a dword
  unsigned chk[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) chk[j] = foff[j] != FAR ? TAGS : 0u;
  // LDS: partial of source wave s, element (row, unit): 4 gates = 16 bytes at ((s * 16 + row) * 16 + unit) * 4 floats
  const unsigned wr_base = (unsigned)(((w * 16 + 4 * fq) * 16 + fr) * 4);              // + rr * 64 floats, + parity * 4096
  const unsigned rd_base = (unsigned)((row * 16 + fr) * 4);                              // + s * 1024 floats, + parity * 4096

  bool dead = false;                                    // a poll of this wave timed out (or the launch was aborted): stop waiting
  float sv[6];
  constexpr bool no_stash = NST == 1;
  auto flush = [&](int ps, f32x4& Pp) {
    const int t = dir ? T - 1 - ps : ps;
    const bool act = t < len;
    if (!no_stash) {
      stf4(rg, act ? og + (unsigned)t * sg : OOB, f32x4{sv[0], sv[1], sv[2], sv[3]});
      stf(rc, inb ? oc + (unsigned)t * scc : OOB, sv[4]);        // rows past their length carry the frozen state (never read)
    }
    stf(rh, inb ? oh + (unsigned)t * sc : OOB, sv[5]);           // zero at padded positions (pad_packed_sequence)
    load_pre(Pp, ps + 2);
  };
  bool fast = false;
  const unsigned xcc = my_xcc_id() ^ ((L.xcd_local == 3 && (ht & 1)) ? 8u : 0u);
  if (L.xcd_local && tid == 0)
    __hip_atomic_store((gu64*)(my_line + 48), ((unsigned long long)xcc << 32) | L.epoch_base, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);

  auto do_step = [&](int step, f32x4& P, f32x4& Pp, auto first_tag, auto fm_tag) {
    constexpr bool FIRST = decltype(first_tag)::value;
    constexpr int FM = decltype(fm_tag)::value;
    const int t = dir ? T - 1 - step : step;
    const unsigned epoch = L.epoch_base + (unsigned)step + 1u;
    f32x4 z = P;
    if (!FIRST) {
      const unsigned need = epoch - 1u;
      const unsigned par = (need & 1u) * slot_b;
      const unsigned tm = ((need >> 1) & 1u) ? TAGS : 0u;           // the tag bits the image of epoch `need` carries
      u32x4 fa[3];
      if (FM == 0) {                                     // steps 1 and 2: flags (the image may hold a previous launch's tags)
        if (!dead) {
          const bool ok = poll_tiles4(fr4, aoff, abort_w, awatch, need);
          if (!ok) { dead = true; if (lane == 0) st_flag(abort_w, 1u); }
        }
        if (L.xcd_local && step == 1) {
          const unsigned long long v = __hip_atomic_load((const gu64*)(flags + (size_t)((awatch ? lane : 0) * 2 + mt) * 64 + 48), __ATOMIC_RELAXED,
                                                         __HIP_MEMORY_SCOPE_AGENT);
          fast = __all(!awatch || v == (((unsigned long long)xcc << 32) | L.epoch_base));
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) fa[j] = ld16_sc1(xr, par + foff[j]);
      } else {                                           // steady state: the fragments themselves say when they are there
        // (one copy of the three loads in flight: see the note at POLL_SLEEP)
        u32x4 fs[3];
        // the fragments with the expected tag XORed off (what the MFMAs take); an element that still carries the other tag keeps a tag
        // bit -- `stale` -- and a nonexistent tile reads as zero and stays zero (cl = 0)
        auto untag = [&](u32x4 (&x)[3], const u32x4 (&f)[3]) {
          unsigned t = 0;
#pragma unroll
          for (int j = 0; j < 3; ++j) {
            const unsigned cl = chk[j] ? tm : 0u;
#pragma unroll
            for (int i = 0; i < 4; ++i) { x[j][i] = f[j][i] ^ cl; t |= x[j][i]; }
          }
          return (t & TAGS) != 0;
        };
#pragma unroll
        for (int j = 0; j < 3; ++j) fs[j] = ld16_sc1(xr, par + foff[j]);
        bool got = false;
        for (unsigned spins = 0; !got; ++spins) {
          if (!__any(untag(fa, fs)) || dead) {
            got = true;
          } else {
            __builtin_amdgcn_s_sleep(POLL_SLEEP);           // a short pause before asking again (see POLL_SLEEP)
#pragma unroll
            for (int j = 0; j < 3; ++j) fs[j] = ld16_sc1(xr, par + foff[j]);
          }
          if (!got && (spins > SPIN_LIMIT || ((spins & 255u) == 0 && spins && ld_flag(abort_w) != 0))) {
            dead = true; got = true;
            if (lane == 0) st_flag(abort_w, 1u);
          }
        }
      }
      if (FM == 0) {                                     // (flag steps: tags off here)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const unsigned cl = chk[j] ? tm : 0u;
#pragma unroll
          for (int i = 0; i < 4; ++i) fa[j][i] ^= cl;
        }
      }
      bf16x8 af[3];
#pragma unroll
      for (int j = 0; j < 3; ++j) af[j] = __builtin_bit_cast(bf16x8, fa[j]);
      f32x4 acc[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        if (w + 4 * j < KS) {                            // wave-uniform
#pragma unroll
          for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[j], wreg[g][j], acc[g], 0, 0, 0);
        }
      }
      float* wr = red + (step & 1) * 4096 + wr_base;
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) *reinterpret_cast<f32x4*>(wr + rr * 64) = f32x4{acc[0][rr], acc[1][rr], acc[2][rr], acc[3][rr]};
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
      const float* rd = red + (step & 1) * 4096 + rd_base;
      const f32x4 v0 = *reinterpret_cast<const f32x4*>(rd), v1 = *reinterpret_cast<const f32x4*>(rd + 1024);
      const f32x4 v2 = *reinterpret_cast<const f32x4*>(rd + 2048), v3 = *reinterpret_cast<const f32x4*>(rd + 3072);
#pragma unroll
      for (int g = 0; g < 4; ++g) z[g] = (((v0[g] + v1[g]) + v2[g]) + v3[g]) + P[g];
    }
    {
      const bool act = t < len;
      const float gi = sigmoid_fast(z[0]);
      const float gf = sigmoid_fast(z[1]);
      float gg, go, cn, hn;
      if (CELL == MMDA_CELL_GRU) {       // four-slot GRU (see lstm.hip): slots r, z, x-part of n, h-part of n; stash [r, z, n, q], h
        go = z[3];
        gg = tanh_fast(z[2] + gi * go);
        hn = (1.f - gf) * gg + gf * h_reg;
        cn = hn;
      } else {
        gg = tanh_fast(z[2]);
        go = sigmoid_fast(z[3]);
        cn = gf * c_reg + gi * gg;
        hn = go * tanh_fast(cn);
      }
      c_reg = act ? cn : c_reg;
      h_reg = act ? hn : h_reg;
      sv[0] = gi; sv[1] = gf; sv[2] = gg; sv[3] = go; sv[4] = c_reg; sv[5] = act ? hn : 0.f;
    }
    if (step + 1 < T) {
      const unsigned par = (epoch & 1u) * slot_b;
      const bool fst = FM == 0 ? fast : FM == 1;
      // |h| < 1, so bit 14 of its bf16 form is free: it carries bit 1 of the epoch -- the value alternates between the successive
      // uses of an image (epochs e, e + 2, ...) and lets a reader tell, element by element, that what it fetched is this step's
      const short hv = (short)(f2bf(h_reg) | (((epoch >> 1) & 1u) << 14));
      if (fst) __builtin_amdgcn_raw_buffer_store_b16(hv, xr, par + pub_off, 0, 0);
      else __builtin_amdgcn_raw_buffer_store_b16(hv, xr, par + pub_off, 0, 16);
      if (FM == 0 && step < 2) {                         // steps 0 and 1 are announced by flag as well (read by steps 1 and 2)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");             // this wave's stores have landed (in L2 / written through)
        if (lane == 0) { if (fst) st_flag_plain(my_flag, epoch); else st_flag(my_flag, epoch); }
      }
    }
    // the stash of THIS step and the pre-activations of step + 2 (into the buffer this step used), behind the publish: the wave has
    // nothing to do until its neighbours' h arrives
    flush(step, P);
    (void)Pp;
  };
  {
    typedef std::integral_constant<bool, true> TrueT;
    typedef std::integral_constant<bool, false> FalseT;
    typedef std::integral_constant<int, 0> FmVar;
    typedef std::integral_constant<int, 1> FmLocal;
    typedef std::integral_constant<int, 2> FmThrough;
    int step = 0;
    if (T > 0) { do_step(0, pre[0], pre[1], TrueT{}, FmVar{}); step = 1; }
    if (T > 1) { do_step(1, pre[1], pre[0], FalseT{}, FmVar{}); step = 2; }
    if (T > 2) { do_step(2, pre[0], pre[1], FalseT{}, FmVar{}); step = 3; }
    if (fast) {
      for (; step + 1 < T; step += 2) {
        do_step(step, pre[1], pre[0], FalseT{}, FmLocal{});
        do_step(step + 1, pre[0], pre[1], FalseT{}, FmLocal{});
      }
      if (step < T) { do_step(step, pre[1], pre[0], FalseT{}, FmLocal{}); ++step; }
    } else {
      for (; step + 1 < T; step += 2) {
        do_step(step, pre[1], pre[0], FalseT{}, FmThrough{});
        do_step(step + 1, pre[0], pre[1], FalseT{}, FmThrough{});
      }
      if (step < T) { do_step(step, pre[1], pre[0], FalseT{}, FmThrough{}); ++step; }
    }
  }
  // final hidden state straight into the utterance layout [h1_fwd, h2_fwd, h1_bwd, h2_bwd] (models.py:203)
  if (inb) D.utt[(int64_t)b * 4 * H + (dir * 2 + D.layer) * H + col] = h_reg;
}

// ------------------------------------------------------------------------------------------------ backward, four waves per tile
// The same split for dh_{t-1} = dG_t W_hh (see lstm_bwd_wave_kernel for the reduce-scatter this implements).  The workgroup of a
// (m-tile, hidden tile) owns the gate gradients of its 16 x 16 elements:
//   gather   wave w sums the partial dh of rows 4w..4w+3 over all producers.  The image is the write-through form of the wave kernel
//            ([consumer tile][m-tile][producer][lane] x 8 B, a lane's 8 bytes = rows 4 fq..+3 of unit fr), so those rows are 128
//            contiguous bytes per producer: lane (producer slot pl = lane >> 3, unit pair uc = lane & 7) fetches 16 bytes (two units
//            x four rows) of producers pl, pl + 8, pl + 16, adds them in fp32, and a three-stage reduce-scatter across the eight
//            producer slots (lane bits 5, 4, 3) leaves every lane with the sum of ONE element: unit 2 uc + bit 5, row 2 bit 4 + bit 3
//   cell     one element per lane, factors prepared at the end of the previous step (derive)
//   dG tile  16 x 64 bf16 through LDS (each wave writes its four rows, ONE workgroup barrier per step, double buffered)
//   MFMA     wave w multiplies the tile with the W_hh columns of hidden tiles w, w+4, ... (<= 5 tiles, 10 MFMAs), publishes them
// Hand-off without flags, as in the forward kernel -- except that a partial dh has no spare bit of its own: the dG tile is scaled
// by 2^-32 on its way to the matrix cores (a power of two: exact), so that every published bf16 partial is below 2 in magnitude
// and its bit 14 is free for the epoch tag; the gatherer multiplies the fp32 sum by 2^32.  (Gradients beyond 2^33 -- or NaN -- read
// as a tag that never matches or matches early: the first times out into the abort word, both belong to a diverged run.)
// value of lane (l ^ 32) / (l ^ 16) / (l ^ 8).  v_permlane32_swap(x, x) returns (x[l], x[l + 32]) in the lower and (x[l - 32], x[l]) in the
// upper half of the wave; v_permlane16_swap likewise per pair of 16-lane rows; row_ror:8 rotates a row of 16 by 8.
typedef unsigned u2x __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float lane_xor32(float v, bool upper) {
  const u2x r = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, v), __builtin_bit_cast(unsigned, v), false, false);
  return __builtin_bit_cast(float, upper ? r[0] : r[1]);
}
__device__ __forceinline__ float lane_xor16(float v, bool odd_row) {
  const u2x r = __builtin_amdgcn_permlane16_swap(__builtin_bit_cast(unsigned, v), __builtin_bit_cast(unsigned, v), false, false);
  return __builtin_bit_cast(float, odd_row ? r[0] : r[1]);
}
__device__ __forceinline__ float lane_xor8(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x128 /* row_ror:8 */, 0xf, 0xf, true));
}

template <int CELL, int HDH, int D16>
__global__ __launch_bounds__(256, 4) void lstm_bwd_quad_kernel(CLaunch L) {   // (<= 128 registers: four workgroups share a CU at large batches)
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __builtin_amdgcn_s_setprio(3);
  const int role = L.blk2role[blockIdx.x];
  if (role < 0) return;
  Where wh;
  wh.di = 0;
#pragma unroll
  for (int i = 1; i < MAXD; ++i)
    if (i < L.n && role >= L.d[i].wg_begin) wh.di = i;
  const CDesc& D = L.d[wh.di];
  {
    const int local = role - D.wg_begin;
    wh.dir = local / (L.ng * D.NCw);
    const int rem = local % (L.ng * D.NCw);
    wh.grp = L.g0 + rem / D.NCw;
    wh.me = rem % D.NCw;
  }
  const int H = D.H, Hp = D.Hp, nHT = D.nHT, NC = D.NC;
  const int B = L.B, T = L.T, dir = wh.dir;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int fr = lane & 15, fq = lane >> 4;             // MFMA frame
  const int rho = wh.me;
  const int mt = rho & 1, ht = rho >> 1;
  // cell frame: the element the reduce-scatter leaves in this lane
  const int uc = lane & 7, pl = lane >> 3;
  const bool b3 = (lane >> 3) & 1, b4 = (lane >> 4) & 1, b5 = (lane >> 5) & 1;
  const int cu = 2 * uc + (b5 ? 1 : 0), crow = 2 * (b4 ? 1 : 0) + (b3 ? 1 : 0);
  const int row = 4 * w + crow, b = wh.grp * GROUP + mt * 16 + row, col = ht * 16 + cu;
  const int ngt = (B + GROUP - 1) / GROUP;
  const unsigned G4 = 4u * H;
  unsigned short* Tr = reinterpret_cast<unsigned short*>(smem);       // [parity][16 rows][64 gate columns] bf16

  unsigned char* abort_w = D.xchg;
  unsigned char* flags = D.xchg + xchg_flags_off() + ((size_t)(dir * ngt + wh.grp) * NC) * FLAG_STRIDE;
  unsigned char* Xb = D.xchg + xchg_x_off(ngt, NC) + ((size_t)(dir * ngt + wh.grp) * 2) * xchg_slot(NC, Hp);
  unsigned char* my_line = flags + (size_t)rho * 64;
  unsigned char* my_flag = my_line + 32 + 4 * w;
  const __amdgpu_buffer_rsrc_t fr4 = make_rsrc(flags, (unsigned)(2 * nHT) * 64u);
  const bool awatch = lane < nHT;
  const unsigned aoff = awatch ? (unsigned)(lane * 2 + mt) * 64u + 32u : OOB;

  // W_hh fragments: gate rows of the own hidden tile (two k-steps) x the column tiles w, w + 4, ...
  bf16x8 wreg[5][2];
  {
    const bf16x8* src = reinterpret_cast<const bf16x8*>(D.wpack_c[dir]);
#pragma unroll
    for (int j = 0; j < 5; ++j)
#pragma unroll
      for (int ks2 = 0; ks2 < 2; ++ks2) {
        const int nt = w + 4 * j;
        wreg[j][ks2] = nt < nHT ? src[((size_t)(ht * nHT + nt) * 2 + ks2) * 64 + lane] : bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
      }
  }
  const __amdgpu_buffer_rsrc_t rg = make_rsrc(D.gates, (unsigned)T * B * 2u * G4 * 4u);
  const __amdgpu_buffer_rsrc_t rc = make_rsrc(D.cstash, (unsigned)T * (unsigned)((B + 3) & ~3) * 2u * H * 4u);
  const unsigned scc = (unsigned)((B + 3) >> 2) * 2u * H * 16u;
  const __amdgpu_buffer_rsrc_t rd = make_rsrc(const_cast<float*>(D.d_hseq), D.d_hseq ? (unsigned)T * B * 2u * H * 4u : 0u);
  const unsigned sg = (unsigned)B * 2u * G4 * 4u, sc = (unsigned)B * 2u * H * 4u;
  const bool inb = col < H && b < B;
  const int len = inb ? L.lengths[min(b, B - 1)] : 0;
  const unsigned og = (((unsigned)b * 2u + dir) * G4 + col * 4) * 4u;
  const unsigned oc = ((((((unsigned)b >> 2) * 2u + dir) * H + col) << 2) + ((unsigned)b & 3u)) * 4u;
  const unsigned oh = ((unsigned)b * 2u * H + dir * H + col) * 4u;
  const float d_fin = inb ? D.utt[(size_t)b * 4u * H + (dir * 2 + D.layer) * H + col] : 0.f;
  float dc = 0.f;
  struct Raw { f32x4 g; float cp, dh; } raw;
  struct Dv { float a[6], dh; } dv;
  float c_keep = 0.f;
  const bool has_dh = HDH == 2 ? D.d_hseq != nullptr : HDH == 1;
  auto load_raw = [&](int step) {
    const int t = dir ? step : T - 1 - step;
    const int tp = dir ? t + 1 : t - 1;
    const bool act = step < T && t < len;
    raw.g = ldf4(rg, act ? og + (unsigned)t * sg : OOB);
    raw.cp = ldf(rc, (step < T && tp >= 0 && tp < len) ? oc + (unsigned)tp * scc : OOB);
    raw.dh = has_dh ? ldf(rd, act ? oh + (unsigned)t * sc : OOB) : 0.f;
  };
  auto derive = [&](int step) {                         // see lstm_bwd_wave_kernel
    const int t = dir ? step : T - 1 - step;
    const bool act = step < T && t < len;
    const bool fin = dir ? (t == 0) : (t == len - 1);
    const float gi = raw.g[0], gf = raw.g[1], gg = raw.g[2], go = raw.g[3];
    dv.dh = raw.dh + ((act && fin) ? d_fin : 0.f);
    if (CELL == MMDA_CELL_GRU) {
      dv.a[0] = act ? (1.f - gf) * (1.f - gg * gg) : 0.f;
      dv.a[1] = go * gi * (1.f - gi);
      dv.a[2] = (raw.cp - gg) * gf * (1.f - gf);
      dv.a[3] = gi;
      dv.a[4] = 0.f;
      dv.a[5] = gf;
    } else {
      const float tc = tanh_fast(c_keep);
      dv.a[0] = gg * gi * (1.f - gi);
      dv.a[1] = raw.cp * gf * (1.f - gf);
      dv.a[2] = gi * (1.f - gg * gg);
      dv.a[3] = tc * go * (1.f - go);
      dv.a[4] = go * (1.f - tc * tc);
      dv.a[5] = gf;
      c_keep = raw.cp;
    }
  };
  if (CELL == MMDA_CELL_LSTM) {
    const int t0 = dir ? 0 : T - 1;
    c_keep = ldf(rc, t0 < len ? oc + (unsigned)t0 * scc : OOB);
  }
  load_raw(0);
  derive(0);
  load_raw(1);
  const unsigned slot_b = (unsigned)xchg_slot(NC, Hp);
  const unsigned RS = (unsigned)((nHT + 1) & ~1) * 512u;
  const unsigned img_b = (unsigned)(nHT * 2) * RS;
  const __amdgpu_buffer_rsrc_t xr = make_rsrc(Xb, slot_b + img_b);
  constexpr unsigned TAGS = 0x40004000u;
  unsigned goff[3], chk[3];
#pragma unroll
  for (int l = 0; l < 3; ++l) {
    const int p = pl + 8 * l;
    goff[l] = p < nHT ? (unsigned)(ht * 2 + mt) * RS + (unsigned)p * 512u + (unsigned)w * 128u + (unsigned)uc * 16u : FAR;
    chk[l] = p < nHT ? TAGS : 0u;
  }
  const unsigned pub_base = (unsigned)mt * RS + (unsigned)(ht * 64 + lane) * 8u;         // + consumer tile nt * pub_stride
  const unsigned pub_stride = 2u * RS;

  bool dead = false;
  typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;
  float dgv[4];
  const __amdgpu_buffer_rsrc_t rg16 = make_rsrc(D.dg16, D.dg16 ? (unsigned)T * B * 2u * G4 * 2u : 0u);
  const bool has_dg16 = D16 == 2 ? D.dg16 != nullptr : true;
  const bool f32_dg = D16 == 2 ? !(has_dg16 && D.dg16_only) : false;
  auto flush = [&](int ps) {
    const int t = dir ? ps : T - 1 - ps;
    const unsigned o = inb ? og + (unsigned)t * sg : OOB;               // zero at padded positions too
    if (f32_dg) stf4(rg, o, f32x4{dgv[0], dgv[1], dgv[2], dgv[3]});
    if (has_dg16) {
      const u32x2 pk = {pack_bf16x2(dgv[0], dgv[1]), pack_bf16x2(dgv[2], dgv[3])};
      __builtin_amdgcn_raw_buffer_store_b64(pk, rg16, inb ? (og + (unsigned)t * sg) >> 1 : OOB, 0, STASH_AUX);
    }
  };
  bool fast = false;
  const unsigned xcc = my_xcc_id() ^ ((L.xcd_local == 3 && (ht & 1)) ? 8u : 0u);
  if (L.xcd_local && tid == 0)
    __hip_atomic_store((gu64*)(my_line + 48), ((unsigned long long)xcc << 32) | L.epoch_base, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const float up = 4294967296.f, down = 1.f / 4294967296.f;            // 2^32, 2^-32

  auto do_step = [&](int step, auto first_tag, auto fm_tag) {
    constexpr bool FIRST = decltype(first_tag)::value;
    constexpr int FM = decltype(fm_tag)::value;
    const unsigned epoch = L.epoch_base + (unsigned)step + 1u;
    float dh_rec = 0.f;
    if (!FIRST) {
      const unsigned need = epoch - 1u;
      const unsigned par = (need & 1u) * slot_b;
      const unsigned tm = ((need >> 1) & 1u) ? TAGS : 0u;
      u32x4 fa[3];
      if (FM == 0) {
        if (!dead) {
          const bool ok = poll_tiles4(fr4, aoff, abort_w, awatch, need);
          if (!ok) { dead = true; if (lane == 0) st_flag(abort_w, 1u); }
        }
        if (L.xcd_local && step == 1) {
          const unsigned long long v = __hip_atomic_load((const gu64*)(flags + (size_t)((awatch ? lane : 0) * 2 + mt) * 64 + 48), __ATOMIC_RELAXED,
                                                         __HIP_MEMORY_SCOPE_AGENT);
          fast = __all(!awatch || v == (((unsigned long long)xcc << 32) | L.epoch_base));
        }
#pragma unroll
        for (int l = 0; l < 3; ++l) fa[l] = ld16_sc1(xr, par + goff[l]);
      } else {
        u32x4 fs[3];                                     // (see the forward kernel)
        auto untag = [&](u32x4 (&x)[3], const u32x4 (&f)[3]) {
          unsigned t = 0;
#pragma unroll
          for (int l = 0; l < 3; ++l) {
            const unsigned cl = chk[l] ? tm : 0u;
#pragma unroll
            for (int i = 0; i < 4; ++i) { x[l][i] = f[l][i] ^ cl; t |= x[l][i]; }
          }
          return (t & TAGS) != 0;
        };
#pragma unroll
        for (int l = 0; l < 3; ++l) fs[l] = ld16_sc1(xr, par + goff[l]);
        bool got = false;
        for (unsigned spins = 0; !got; ++spins) {
          if (!__any(untag(fa, fs)) || dead) {
            got = true;
          } else {
            __builtin_amdgcn_s_sleep(POLL_SLEEP);           // a short pause before asking again (see POLL_SLEEP)
#pragma unroll
            for (int l = 0; l < 3; ++l) fs[l] = ld16_sc1(xr, par + goff[l]);
          }
          if (!got && (spins > SPIN_LIMIT || ((spins & 255u) == 0 && spins && ld_flag(abort_w) != 0))) {
            dead = true; got = true;
            if (lane == 0) st_flag(abort_w, 1u);
          }
        }
      }
      if (FM == 0) {                                     // (flag steps: tags off here)
#pragma unroll
        for (int l = 0; l < 3; ++l) {
          const unsigned cl = chk[l] ? tm : 0u;
#pragma unroll
          for (int i = 0; i < 4; ++i) fa[l][i] ^= cl;
        }
      }
      flush(step - 1);
      load_raw(step + 1);                                // consumed by derive() at the end of this step
      // a[unit bit * 4 + row] of units 2 uc, 2 uc + 1, summed over this lane's producers in the order pl, pl + 8, pl + 16
      float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int l = 0; l < 3; ++l) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const unsigned x = fa[l][q];                   // (tags already off)
          a[2 * q] += __builtin_bit_cast(float, x << 16);
          a[2 * q + 1] += __builtin_bit_cast(float, x & 0xffff0000u);
        }
      }
      // reduce-scatter over the producer slots: bit 5 picks the unit, bits 4 and 3 the row.  The partner's value comes by
      // v_permlane32_swap / v_permlane16_swap / a DPP row rotation (VALU, a few cycles each; three dependent ds_bpermute round trips
      // were ~0.15 us of every step: tools/micro/permlane_swap.hip pins the swap semantics)
      float k4[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float keep = b5 ? a[4 + i] : a[i], send = b5 ? a[i] : a[4 + i];
        k4[i] = keep + lane_xor32(send, b5);
      }
      float k2[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const float keep = b4 ? k4[2 + i] : k4[i], send = b4 ? k4[i] : k4[2 + i];
        k2[i] = keep + lane_xor16(send, b4);
      }
      {
        const float keep = b3 ? k2[1] : k2[0], send = b3 ? k2[0] : k2[1];
        dh_rec = (keep + lane_xor8(send)) * up;
      }
    }
    // gate gradients of the lane's element: linear in dh / dc with the factors derive() prepared
    {
      float dh = dh_rec + dv.dh;
      float dp[4];
      if (CELL == MMDA_CELL_GRU) {
        dh += dc;
        const float dpn = dh * dv.a[0];
        dp[0] = dpn * dv.a[1];
        dp[1] = dh * dv.a[2];
        dp[2] = dpn;
        dp[3] = dpn * dv.a[3];
        dc = dh * dv.a[5];
      } else {
        const float dct = dc + dh * dv.a[4];
        dp[0] = dct * dv.a[0];
        dp[1] = dct * dv.a[1];
        dp[2] = dct * dv.a[2];
        dp[3] = dh * dv.a[3];
        dc = dct * dv.a[5];
      }
      unsigned short* tr = Tr + (step & 1) * 1024 + row * 64 + cu;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        tr[g * 16] = f2bf(dp[g] * down);
        dgv[g] = dp[g];
      }
    }
    if (step + 1 < T) {
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
      const unsigned short* tr = Tr + (step & 1) * 1024;
      const bf16x8 a0 = *reinterpret_cast<const bf16x8*>(&tr[fr * 64 + fq * 8]);
      const bf16x8 a1 = *reinterpret_cast<const bf16x8*>(&tr[fr * 64 + 32 + fq * 8]);
      const unsigned par = (epoch & 1u) * slot_b;
      const unsigned tg = ((epoch >> 1) & 1u) ? TAGS : 0u;
      f32x4 accs[5];
#pragma unroll
      for (int j = 0; j < 5; ++j) accs[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, wreg[j][0], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
#pragma unroll
      for (int j = 0; j < 5; ++j) accs[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, wreg[j][1], accs[j], 0, 0, 0);
      const bool fst = FM == 0 ? fast : FM == 1;
#pragma unroll
      for (int j = 0; j < 5; ++j) {
        const u32x2 pk = {pack_bf16x2(accs[j][0], accs[j][1]) | tg, pack_bf16x2(accs[j][2], accs[j][3]) | tg};
        const unsigned so = (w + 4 * j) < nHT ? par + (unsigned)(w + 4 * j) * pub_stride : FAR;
        if (fst) __builtin_amdgcn_raw_buffer_store_b64(pk, xr, pub_base + so, 0, 0);
        else __builtin_amdgcn_raw_buffer_store_b64(pk, xr, pub_base + so, 0, 16);
      }
      if (FM == 0 && step < 2) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane == 0) { if (fst) st_flag_plain(my_flag, epoch); else st_flag(my_flag, epoch); }
      }
      derive(step + 1);
    }
  };
  {
    typedef std::integral_constant<bool, true> TrueT;
    typedef std::integral_constant<bool, false> FalseT;
    typedef std::integral_constant<int, 0> FmVar;
    typedef std::integral_constant<int, 1> FmLocal;
    typedef std::integral_constant<int, 2> FmThrough;
    int step = 0;
    if (T > 0) { do_step(0, TrueT{}, FmVar{}); step = 1; }
    if (T > 1) { do_step(1, FalseT{}, FmVar{}); step = 2; }
    if (T > 2) { do_step(2, FalseT{}, FmVar{}); step = 3; }
    if (fast) { for (; step < T; ++step) do_step(step, FalseT{}, FmLocal{}); }
    else { for (; step < T; ++step) do_step(step, FalseT{}, FmThrough{}); }
    if (T > 0) flush(T - 1);
  }
}

}  // namespace

Kernel quad_kernel(int id, bool bwd) {
  constexpr int LSTM = MMDA_CELL_LSTM, GRU = MMDA_CELL_GRU;
  Kernel f = nullptr, b = nullptr;
  switch (id) {
    case MMDA_LSTM_K_FWD_QUAD_NOSTASH: f = lstm_fwd_quad_kernel<LSTM, 1>; break;
    case MMDA_LSTM_K_FWD_QUAD: f = lstm_fwd_quad_kernel<LSTM, 0>; break;
    case MMDA_LSTM_K_FWD_QUAD_GRU_NOSTASH: f = lstm_fwd_quad_kernel<GRU, 1>; break;
    case MMDA_LSTM_K_FWD_QUAD_GRU: f = lstm_fwd_quad_kernel<GRU, 0>; break;
    case MMDA_LSTM_K_BWD_QUAD_PRESENT: b = lstm_bwd_quad_kernel<LSTM, 1, 1>; break;
    case MMDA_LSTM_K_BWD_QUAD_ABSENT: b = lstm_bwd_quad_kernel<LSTM, 0, 1>; break;
    case MMDA_LSTM_K_BWD_QUAD: b = lstm_bwd_quad_kernel<LSTM, 2, 2>; break;
    case MMDA_LSTM_K_BWD_QUAD_GRU: b = lstm_bwd_quad_kernel<GRU, 2, 2>; break;
  }
  return bwd ? b : f;
}

}  // namespace mmda_resident
