// Resident recurrences, Wave form (lstm_resident.h): every wave owns one (m-tile, hidden tile) for the whole sequence, keeps its W_hh
// fragments in registers and hands over by a flag of its own; 1, 2 or 4 waves per block.  Every H <= 320 where the Quad form does
// not apply; LSTM and GRU.  Also here: the stamped instances (DBG) of tools/diag_lstm_phases.py and the backward PAIR instances.
#include "lstm_resident.h"
#include <type_traits>

namespace mmda_resident {
namespace {

// Flag poll of the wave-autonomous kernels: lane tau watches the flag of hidden tile tau.  One read in flight: round 1 kept four in
// flight ~130 cycles apart to cut the quantisation of the wait, but every read in flight queues in the polling CU's memory pipeline in
// front of the loads that fetch the data (measured below).  Returns false on timeout / abort (bounded spin).
// (flag reads in flight per polling wave: B=256, all eight groups in one launch, step 2.375 ms with four, 2.354 with two, 2.338 with one)
__device__ __forceinline__ bool poll_tiles(const unsigned char* poll_flag, const unsigned char* abort_w, bool watching, unsigned need) {
  for (unsigned spins = 0;; ++spins) {
    const unsigned f = ld_flag(poll_flag);
    if (__all(!watching || (int)(f - need) >= 0)) return true;
    if (spins > SPIN_LIMIT || ((spins & 255u) == 0 && spins && ld_flag(abort_w) != 0)) return false;
  }
}

// XCD-local hand-off (wave-autonomous kernels).  A wave exchanges data only with the waves of its own m-tile (19 for text), and
// the host places those on block ids that are equal mod 8, which the dispatcher has been observed -- not promised -- to deal
// to one XCD.  When that holds the exchange can stay inside that XCD's L2: plain stores keep their lines there (sc1 stores write
// through and drop them, so that even a same-XCD reader pays the cross-XCD latency) and the readers' sc1 loads are L2-served.
// Because the placement is not a contract the waves CHECK it: each stores {launch epoch, XCC_ID} next to its flag before its first
// (write-through) publish; at step 1, after the usual poll, every wave reads the ids of all tiles of its m-tile and switches to
// the plain-store form only if they all equal its own.  All waves of the m-tile read the same words, so they agree.
__device__ __forceinline__ void xcc_announce(unsigned char* my_flag, unsigned epoch_base, unsigned xcc) {
  __hip_atomic_store((gu64*)(my_flag + 8), ((unsigned long long)xcc << 32) | epoch_base, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ bool xcc_all_local(const unsigned char* tile_flag, bool watching, unsigned epoch_base, unsigned xcc) {
  const unsigned long long v = __hip_atomic_load((const gu64*)(tile_flag + 8), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return __all(!watching || v == (((unsigned long long)xcc << 32) | epoch_base));
}

// ------------------------------------------------------------------------------------------------ forward, wave-autonomous form
// Same cluster, same math, no workgroup barrier and no LDS staging.  Every wave owns one (16-sample m-tile, 16-unit hidden
// tile) for the whole sequence and runs on its own:
//   poll    lanes 0..nHT-1 each read the flag of one hidden tile of THIS m-tile (one load instruction covers the cluster)
//   gather  the exchange image is TILE-MAJOR: [hidden tile][m-tile][16 rows][16 units] bf16, 512 contiguous bytes per tile.  The
//           A operand of k-step ks is h[m-tile rows][32ks .. 32ks+31] = tiles 2ks and 2ks+1; in fragment order a lane needs the
//           16 bytes at (row = lane & 15, units 8 (lane >> 4) ..+7): ONE 16-byte sc1 load per lane and k-step straight into the
//           MFMA operand registers -- the gathered h never touches LDS; tiles past the last one read as zero (OOB offset)
//   MFMA    W_hh fragments resident in registers (wreg), counted waits let the MFMAs start as fragments land
//   cell    lane-local, as before
//   publish the wave's 16 x 16 bf16 tile goes through 512 B of wave-private LDS (fragment order -> row order) and out as 32
//           16-byte write-through stores covering whole 64-byte sectors; the wave drains them and raises ITS OWN flag
//           (line m-tile*2 + local tile of its workgroup's flag block)
// NST: compile-time knowledge of "no stash" (evaluation pass): 0 = stash, 1 = none, 2 = decided at run time
template <int KSM, bool GM, int CELL, bool DBG, int NST = 2>
__global__ __launch_bounds__(256, 1) void lstm_fwd_wave_kernel(CLaunch L) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __builtin_amdgcn_s_setprio(3);
  const int role = L.blk2role[blockIdx.x];
  if (role < 0) return;
  // role -> (descriptor, direction, batch group, first wave-role of this block); wave-role rho = (hidden tile, m-tile)
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
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  __builtin_amdgcn_s_setprio(3);         // a serial chain: win issue arbitration against whatever else shares the CU
  const int fr = lane & 15, fq = lane >> 4;
  const int rho = wh.me * L.wpb + wave;
  const int mt = rho & 1, ht = rho >> 1;
  if (ht >= nHT) return;                                // no tile: nothing to compute, nobody waits for this wave
  const int col = ht * 16 + fr;
  const int ngt = (B + GROUP - 1) / GROUP;
  const unsigned G4 = 4u * H;
  constexpr bool gm = GM;
  unsigned short* Tr = reinterpret_cast<unsigned short*>(smem) + wave * 256;      // 16 x 16 bf16, wave-private

  unsigned char* abort_w = D.xchg;
  unsigned char* flags = D.xchg + xchg_flags_off() + ((size_t)(dir * ngt + wh.grp) * NC) * FLAG_STRIDE;
  unsigned char* Xb = D.xchg + xchg_x_off(ngt, NC) + ((size_t)(dir * ngt + wh.grp) * 2) * xchg_slot(NC, Hp);
  // one 64-byte flag line per wave-role (the block of NC * FLAG_STRIDE bytes holds >= 2 * nHT lines)
  unsigned char* my_flag = flags + (size_t)rho * 64;
  // lane tau < nHT polls the flag of hidden tile tau for this m-tile
  const int tau = lane < nHT ? lane : 0;
  const unsigned char* poll_flag = flags + (size_t)(tau * 2 + mt) * 64;

  bf16x8 wreg[4][KSM];
  {
    const bf16x8* src = reinterpret_cast<const bf16x8*>(D.wpack[dir]);
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int k2 = 0; k2 < KSM; ++k2)
        wreg[g][k2] = k2 < KS ? src[((size_t)(ht * 4 + g) * KS + k2) * 64 + lane] : bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
  }
  const __amdgpu_buffer_rsrc_t rg = make_rsrc(D.gates, (unsigned)T * B * 2u * G4 * 4u);
  // cell-state stash: (T,B,2,H) fp32; with the gate-minor layout it is batch-minor-by-4, (T, ceil(B/4), 2, H, 4): the four samples a
  // lane owns are 16 contiguous bytes (one access in the wave-autonomous kernels instead of four)
  const __amdgpu_buffer_rsrc_t rc = make_rsrc(D.cstash, (unsigned)T * (GM ? (unsigned)((B + 3) & ~3) : (unsigned)B) * 2u * H * 4u);
  const unsigned scc = GM ? (unsigned)((B + 3) >> 2) * 2u * H * 16u : (unsigned)B * 2u * H * 4u;      // its byte stride per time step
  const __amdgpu_buffer_rsrc_t rh = make_rsrc(D.hseq, (unsigned)T * B * 2u * H * 4u);
  const unsigned sg = (unsigned)B * 2u * G4 * 4u, sc = (unsigned)B * 2u * H * 4u;
  unsigned og[4], oc[4], oh[4];
  int len_r[4];
  bool inb[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int b = wh.grp * GROUP + mt * 16 + fq * 4 + r;
    inb[r] = col < H && b < B;
    const int lv = L.lengths[min(b, B - 1)];
    len_r[r] = inb[r] ? lv : 0;
    og[r] = (((unsigned)b * 2u + dir) * G4 + (gm ? col * 4 : col)) * 4u;
    oc[r] = GM ? ((((((unsigned)b >> 2) * 2u + dir) * H + col) << 2) + ((unsigned)b & 3u)) * 4u : (((unsigned)b * 2u + dir) * H + col) * 4u;
    oh[r] = ((unsigned)b * 2u * H + dir * H + col) * 4u;
  }
  float c_reg[4] = {0.f, 0.f, 0.f, 0.f}, h_reg[4] = {0.f, 0.f, 0.f, 0.f};
  float pre[2][4][4];
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
  // ONE descriptor over both parity images (selecting between two descriptors per step makes hipcc keep them in VGPRs and
  // wrap every access in a readfirstlane loop); the parity picks a byte offset instead
  const unsigned slot_b = (unsigned)xchg_slot(NC, Hp);
  const unsigned img_b = (unsigned)nHT * 2u * 512u;
  const __amdgpu_buffer_rsrc_t xr = make_rsrc(Xb, slot_b + img_b);
  // fragment of k-step ks: tile 2ks + (fq >> 1), row fr, units 8 (fq & 1) ..+7
  // = frag_base + k2 * 2048 bytes; the second tile of the last k-step may not exist (odd tile count): those lanes read zero
  const unsigned frag_base = (unsigned)(((((fq >> 1) * 2 + mt) * 256) + fr * 16 + 8 * (fq & 1)) * 2);
  const unsigned pub_off = lane < 32 ? (unsigned)((((ht * 2 + mt) * 256) + lane * 8) * 2) : OOB;

  unsigned long long ph[8] = {0, 0, 0, 0, 0, 0, 0, 0}, last = 0;
#define STAMP(i) do { if (DBG && L.dbg && tid == 0) { unsigned long long now_ = __builtin_readcyclecounter(); ph[i] += now_ - last; last = now_; } } while (0)
  if (DBG && L.dbg && tid == 0) last = __builtin_readcyclecounter();

  bool alive = true;
  float sv[4][6];                                       // stash of the previous step, flushed behind the next step's fragment loads
  // off the chain: the stash of step `ps` for the backward pass and the pre-activations of step ps + 2 into the buffer that
  // step used.  Issued right after a step's fragment loads (in front of the poll they would delay every wave's flag reads).
  const bool no_stash = NST == 2 ? L.no_stash != 0 : NST == 1;      // launch-uniform
  auto flush = [&](int ps, float (&Pp)[4][4]) {
    const int t = dir ? T - 1 - ps : ps;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool act = t < len_r[r];
      const unsigned o = (act && !no_stash) ? og[r] + (unsigned)t * sg : OOB;
      if (!no_stash) {
        if (gm) {
          stf4(rg, o, f32x4{sv[r][0], sv[r][1], sv[r][2], sv[r][3]});
        } else {
          stf(rg, o, sv[r][0]); stf(rg, act ? o + H * 4u : OOB, sv[r][1]); stf(rg, act ? o + 2u * H * 4u : OOB, sv[r][2]);
          stf(rg, act ? o + 3u * H * 4u : OOB, sv[r][3]);
        }
        if (!gm) stf(rc, act ? oc[r] + (unsigned)t * scc : OOB, sv[r][4]);
      }
      stf(rh, inb[r] ? oh[r] + (unsigned)t * sc : OOB, sv[r][5]);     // zero at padded positions (pad_packed_sequence)
    }
    // batch-minor stash: the lane's four samples in one 16-byte store (rows past their length carry the frozen state: never read)
    if (gm && !no_stash) stf4(rc, inb[0] ? oc[0] + (unsigned)t * scc : OOB, f32x4{sv[0][4], sv[1][4], sv[2][4], sv[3][4]});
    load_pre(Pp, ps + 2);
  };
  bool fast = false;                                    // XCD-local hand-off in force (wave-uniform, same in every wave of the m-tile)
  const unsigned xcc = my_xcc_id() ^ ((L.xcd_local == 3 && (ht & 1)) ? 8u : 0u);   // (3: test hook, odd tiles announce a wrong id)
  if (L.xcd_local && lane == 0) xcc_announce(my_flag, L.epoch_base, xcc);
  // One time step.  P: pre-activations of this step; Pp: the buffer the previous step used (refilled for step + 1 by flush).
  // FIRST (step 0: h = 0, nothing to wait for) and FM (hand-off form: 0 = the `fast` variable -- steps 0 and 1, before and while the
  // placement is being checked --, 1 = XCD-local for sure, 2 = write-through for sure) are compile-time tags: the steady-state
  // steps carry no step-number or form branches -- every such branch, taken or not, splits the wave's instruction schedule.
  auto do_step = [&](int step, float (&P)[4][4], float (&Pp)[4][4], auto first_tag, auto fm_tag) {
    constexpr bool FIRST = decltype(first_tag)::value;
    constexpr int FM = decltype(fm_tag)::value;
    const int t = dir ? T - 1 - step : step;
    const unsigned epoch = L.epoch_base + (unsigned)step + 1u;
    f32x4 acc[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (!FIRST) {
      // every hidden tile of this m-tile must have published the previous step
      const unsigned need = epoch - 1u;
      alive = poll_tiles(poll_flag, abort_w, lane < nHT, need);
      if (!alive) { if (lane == 0) st_flag(abort_w, 1u); return; }
      if (FM == 0 && L.xcd_local && step == 1) fast = xcc_all_local(poll_flag, lane < nHT, L.epoch_base, xcc);
      STAMP(0);
      const unsigned par = (need & 1u) * slot_b;
      bf16x8 af[KSM];
#pragma unroll
      for (int k2 = 0; k2 < KSM; ++k2)
        af[k2] = __builtin_bit_cast(bf16x8, ld16_sc1(xr, (k2 < KS && 2 * k2 + (fq >> 1) < nHT) ? par + frag_base + (unsigned)k2 * 2048u : OOB));
      flush(step - 1, Pp);
      STAMP(1);
      // (skipping the k-steps past a narrow modality's depth by a wave-uniform test per k-step; issuing all of them on zero operands
      // instead was measured slower)
#pragma unroll
      for (int k2 = 0; k2 < KSM; ++k2) {
        if (k2 < KS) {                                   // workgroup-uniform
#pragma unroll
          for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[k2], wreg[g][k2], acc[g], 0, 0, 0);
        }
      }
      if (DBG && L.dbg) { asm volatile("s_nop 0" :: "v"(acc[0][0]), "v"(acc[1][0]), "v"(acc[2][0]), "v"(acc[3][0])); STAMP(2); }
    }
    // lane-local cell update, branch-free (inactive lanes compute on zeros and are masked by the selects / OOB stores)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool act = t < len_r[r];
      const float gi = sigmoid_fast(acc[0][r] + P[0][r]);
      const float gf = sigmoid_fast(acc[1][r] + P[1][r]);
      float gg, go, cn, hn;
      if (CELL == MMDA_CELL_GRU) {       // four-slot GRU (see lstm.hip): slots r, z, x-part of n, h-part of n; stash [r, z, n, q], h
        go = acc[3][r] + P[3][r];
        gg = tanh_fast(acc[2][r] + P[2][r] + gi * go);
        hn = (1.f - gf) * gg + gf * h_reg[r];
        cn = hn;
      } else {
        gg = tanh_fast(acc[2][r] + P[2][r]);
        go = sigmoid_fast(acc[3][r] + P[3][r]);
        cn = gf * c_reg[r] + gi * gg;
        hn = go * tanh_fast(cn);
      }
      c_reg[r] = act ? cn : c_reg[r];
      h_reg[r] = act ? hn : h_reg[r];
      Tr[(fq * 4 + r) * 16 + fr] = f2bf(h_reg[r]);
      sv[r][0] = gi; sv[r][1] = gf; sv[r][2] = gg; sv[r][3] = go; sv[r][4] = c_reg[r]; sv[r][5] = act ? hn : 0.f;
    }
    if (step + 1 < T) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");            // the tile is complete in the wave-private LDS block
      STAMP(3);
      const unsigned par = (epoch & 1u) * slot_b;
      const u32x4 v = *reinterpret_cast<const u32x4*>(&Tr[(lane & 31) * 8]);
      const bool fst = FM == 0 ? fast : FM == 1;
      if (fst) st16_plain(xr, pub_off == OOB ? OOB : par + pub_off, v);
      else st16_sc1(xr, pub_off == OOB ? OOB : par + pub_off, v);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");               // this wave's stores have landed (in L2 / written through)
      STAMP(4);
      if (lane == 0) { if (fst) st_flag_plain(my_flag, epoch); else st_flag(my_flag, epoch); }
    }
  };
  {
    typedef std::integral_constant<bool, true> TrueT;
    typedef std::integral_constant<bool, false> FalseT;
    typedef std::integral_constant<int, 0> FmVar;
    typedef std::integral_constant<int, 1> FmLocal;
    typedef std::integral_constant<int, 2> FmThrough;
    // pre[0] holds step 0, pre[1] step 1; afterwards flush() refills the buffer of step s - 1 with step s + 1
    int step = 0;
    if (T > 0) { do_step(0, pre[0], pre[1], TrueT{}, FmVar{}); step = 1; }
    if (T > 1 && alive) { do_step(1, pre[1], pre[0], FalseT{}, FmVar{}); step = 2; }
    if (fast) {
      for (; step + 1 < T && alive; step += 2) {
        do_step(step, pre[0], pre[1], FalseT{}, FmLocal{});
        if (alive) do_step(step + 1, pre[1], pre[0], FalseT{}, FmLocal{});
      }
      if (step < T && alive) { do_step(step, pre[0], pre[1], FalseT{}, FmLocal{}); ++step; }
    } else {
      for (; step + 1 < T && alive; step += 2) {
        do_step(step, pre[0], pre[1], FalseT{}, FmThrough{});
        if (alive) do_step(step + 1, pre[1], pre[0], FalseT{}, FmThrough{});
      }
      if (step < T && alive) { do_step(step, pre[0], pre[1], FalseT{}, FmThrough{}); ++step; }
    }
    if (alive && T > 0) flush(T - 1, (T - 1) & 1 ? pre[1] : pre[0]);
  }
  if (DBG && L.dbg && tid == 0)
    for (int i = 0; i < 8; ++i) L.dbg[(size_t)role * 8 + i] = ph[i];
#undef STAMP
  // final hidden state straight into the utterance layout [h1_fwd, h2_fwd, h1_bwd, h2_bwd] (models.py:203)
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int b = wh.grp * GROUP + mt * 16 + fq * 4 + r;
    if (inb[r]) D.utt[(int64_t)b * 4 * H + (dir * 2 + D.layer) * H + col] = h_reg[r];
  }
}

// ------------------------------------------------------------------------------------------------ backward, wave-autonomous form
// dh_{t-1} = dG_t W_hh, reduce-scattered as in the barrier kernel but per WAVE: every wave owns one (m-tile, hidden tile) for
// the whole sequence.  From its own dG (16 samples x 64 gate rows, K = 64: two k-steps, A fragments through 2 KB of
// wave-private LDS) it computes the PARTIAL dh for every hidden tile with W_hh fragments that stay in registers, and
// publishes each 16 x 16 partial in the CONSUMER's accumulator-fragment order (lane: unit lane&15, samples (lane>>4)*4..+3,
// four bf16 = 8 bytes per lane).  The consumer of tile nt reads its nHT partials with one 8-byte sc1 load per lane and
// producer, sums them in fp32 straight in fragment order and runs the lane-local cell backward: no workgroup barrier, no
// LDS staging of gathered data, no transposition on the consumer side.
// HDH / D16: compile-time knowledge of "d_hseq is given" (layer 1) and "dG leaves as bf16 only" (0 / 1; 2 = decided at run time)
// PAIR = 1 (four waves per block, large batches): the two waves of a block that share an m-tile -- hidden tiles 2q and 2q + 1 -- add
// their partial dh tiles in LDS before anything leaves the CU: wave 2q keeps the even consumer tiles, wave 2q + 1 the odd ones, each
// hands the other half of its fp32 accumulators over through 10 KB of LDS (16-byte writes, an epoch word, a bounded spin), adds the
// partner's half and publishes ONE bf16 partial per (consumer tile, producer PAIR).  The exchange image then holds (nHT + 1) / 2
// producers per consumer: half the publish stores and half the gather loads per wave and step.  At B = 256 four waves share a CU's
// address unit and a step is paced by its ~45 vector-memory instructions per wave (4.5 us per step against the forward kernel's
// 2.75 at 26): this takes 19 + 19 of them down to 10 + 10.  (A hidden tile without a partner -- the last of an odd count -- keeps
// and publishes everything itself, as pair nHT / 2.)
template <int NTM, bool GM, int CELL, bool DBG, int HDH = 2, int D16 = 2, int PAIR = 0>
__global__ __launch_bounds__(256, 1) void lstm_bwd_wave_kernel(CLaunch L) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __builtin_amdgcn_s_setprio(3);
  const int role = L.blk2role[blockIdx.x];
  // PAIR: LDS = [4 x 2 KB wave-private dG tiles | 4 x 10 KB hand-over regions | 4 epoch words]
  volatile unsigned* lflag = reinterpret_cast<volatile unsigned*>(smem + 4 * 2048 + 4 * 10240);
  if (PAIR) {
    if ((threadIdx.x & 63) == 0) lflag[threadIdx.x >> 6] = L.epoch_base;      // (LDS is not cleared between launches)
    __syncthreads();                                     // every wave of the block passes here, also the ones that leave below
  }
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
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  __builtin_amdgcn_s_setprio(3);         // a serial chain: win issue arbitration against whatever else shares the CU
  const int fr = lane & 15, fq = lane >> 4;
  const int rho = wh.me * L.wpb + wave;
  const int mt = rho & 1, ht = rho >> 1;
  if (ht >= nHT) return;
  const int col = ht * 16 + fr;
  const int ngt = (B + GROUP - 1) / GROUP;
  const unsigned G4 = 4u * H;
  constexpr bool gm = GM;
  unsigned short* Tr = reinterpret_cast<unsigned short*>(smem) + wave * 1024;     // 16 x 64 bf16, wave-private
  // producer index of this wave in the exchange image, and the number of producers a consumer gathers from
  const int hp = PAIR ? (ht >> 1) : ht;
  const int nP = PAIR ? (nHT + 1) / 2 : nHT;
  const bool has_partner = PAIR && ((ht ^ 1) < nHT);     // (wpb == 4: the partner is wave ^ 2 of this block)
  f32x4* xmine = reinterpret_cast<f32x4*>(smem + 4 * 2048 + wave * 10240) + lane;              // + slot * 64
  const f32x4* xpart = reinterpret_cast<const f32x4*>(smem + 4 * 2048 + (wave ^ 2) * 10240) + lane;

  unsigned char* abort_w = D.xchg;
  unsigned char* flags = D.xchg + xchg_flags_off() + ((size_t)(dir * ngt + wh.grp) * NC) * FLAG_STRIDE;
  unsigned char* Xb = D.xchg + xchg_x_off(ngt, NC) + ((size_t)(dir * ngt + wh.grp) * 2) * xchg_slot(NC, Hp);
  unsigned char* my_flag = flags + (size_t)rho * 64;
  const int tau = lane < nHT ? lane : 0;
  const unsigned char* poll_flag = flags + (size_t)(tau * 2 + mt) * 64;

  // W_hh fragments: gate rows of the own hidden tile (two k-steps) x every column tile nt; cluster-backward packing
  bf16x8 wreg[NTM][2];
  {
    const bf16x8* src = reinterpret_cast<const bf16x8*>(D.wpack_c[dir]);
#pragma unroll
    for (int nt = 0; nt < NTM; ++nt)
#pragma unroll
      for (int ks2 = 0; ks2 < 2; ++ks2)
        wreg[nt][ks2] = nt < nHT ? src[((size_t)(ht * nHT + nt) * 2 + ks2) * 64 + lane] : bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
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
    inb[r] = col < H && b < B;
    const int lv = L.lengths[min(b, B - 1)];
    len_r[r] = inb[r] ? lv : 0;
    og[r] = (((unsigned)b * 2u + dir) * G4 + (gm ? col * 4 : col)) * 4u;
    oc[r] = GM ? ((((((unsigned)b >> 2) * 2u + dir) * H + col) << 2) + ((unsigned)b & 3u)) * 4u : (((unsigned)b * 2u + dir) * H + col) * 4u;
    oh[r] = ((unsigned)b * 2u * H + dir * H + col) * 4u;
    d_fin[r] = ldf(ru, inb[r] ? ((unsigned)b * 4u * H + (dir * 2 + D.layer) * H + col) * 4u : OOB);
  }
  float dc[4] = {0.f, 0.f, 0.f, 0.f};
  // Forward stash of the NEXT step as loaded (raw), and of the current step folded into the factors the gate gradients are
  // linear in (dv): the folding (tanh, products, masks) depends on the stash alone, so it is done at the end of the previous
  // step, while the other waves' partial sums are still on their way; what stays between "partials arrived" and "own partial
  // published" is a handful of multiplies.
  struct Raw { float g[4][4], cp[4], dh[4]; };
  struct Dv { float a[6][4], dh[4]; };
  Raw raw;
  Dv dv;
  float c_keep[4] = {0.f, 0.f, 0.f, 0.f};               // cell state of the step being derived (LSTM)
  const bool has_dh = HDH == 2 ? D.d_hseq != nullptr : HDH == 1;
  auto load_raw = [&](int step) {
    const int t = dir ? step : T - 1 - step;
    const int tp = dir ? t + 1 : t - 1;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool act = step < T && t < len_r[r];
      const unsigned o = og[r] + (unsigned)t * sg;
      if (gm) {
        const f32x4 v = ldf4(rg, act ? o : OOB);
#pragma unroll
        for (int g = 0; g < 4; ++g) raw.g[g][r] = v[g];
      } else {
#pragma unroll
        for (int g = 0; g < 4; ++g) raw.g[g][r] = ldf(rg, act ? o + g * H * 4u : OOB);
      }
      // the state of the step that follows in this walk (= the previous one in time); derive() hands it on as that step's own
      // state, so every state is read once
      if (!gm) raw.cp[r] = ldf(rc, (step < T && tp >= 0 && tp < len_r[r]) ? oc[r] + (unsigned)tp * scc : OOB);
      raw.dh[r] = has_dh ? ldf(rd, act ? oh[r] + (unsigned)t * sc : OOB) : 0.f;      // has_dh is workgroup-uniform
    }
    if (gm) {            // batch-minor stash: the lane's four samples in one 16-byte load; derive() masks the rows past their length
      const f32x4 v = ldf4(rc, (step < T && tp >= 0 && tp < T && inb[0]) ? oc[0] + (unsigned)tp * scc : OOB);
#pragma unroll
      for (int r = 0; r < 4; ++r) raw.cp[r] = v[r];
    }
  };
  // raw (step `step`) + c_keep -> dv.  With dh the total gradient of h_t and dc the carried one:
  //   LSTM: dct = dc + dh a4;  dG = [dct a0, dct a1, dct a2, dh a3];  dc' = dct a5
  //   GRU : dh += dc;          dG = [dh a0 a1, dh a2, dh a0, dh a0 a3];  dc' = dh a5       (stash [r, z, n, q], cp = h_{t-1})
  // Everything is zero at inactive (t >= len) positions: the loads were masked, a0 is masked here.  The carry needs no mask: the
  // inactive steps of a sample come first in this walk (forward direction, carry still zero) or last (reverse direction).
  auto derive = [&](int step) {
    const int t = dir ? step : T - 1 - step;
    const int tpd = dir ? t + 1 : t - 1;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (gm) raw.cp[r] = (tpd >= 0 && tpd < len_r[r]) ? raw.cp[r] : 0.f;     // (the scalar form masked its load instead)
      const bool act = step < T && t < len_r[r];
      const bool fin = dir ? (t == 0) : (t == len_r[r] - 1);
      const float gi = raw.g[0][r], gf = raw.g[1][r], gg = raw.g[2][r], go = raw.g[3][r];
      dv.dh[r] = raw.dh[r] + ((act && fin) ? d_fin[r] : 0.f);
      if (CELL == MMDA_CELL_GRU) {
        dv.a[0][r] = act ? (1.f - gf) * (1.f - gg * gg) : 0.f;
        dv.a[1][r] = go * gi * (1.f - gi);
        dv.a[2][r] = (raw.cp[r] - gg) * gf * (1.f - gf);
        dv.a[3][r] = gi;
        dv.a[4][r] = 0.f;
        dv.a[5][r] = gf;
      } else {
        const float tc = tanh_fast(c_keep[r]);
        dv.a[0][r] = gg * gi * (1.f - gi);
        dv.a[1][r] = raw.cp[r] * gf * (1.f - gf);
        dv.a[2][r] = gi * (1.f - gg * gg);
        dv.a[3][r] = tc * go * (1.f - go);
        dv.a[4][r] = go * (1.f - tc * tc);
        dv.a[5][r] = gf;
        c_keep[r] = raw.cp[r];
      }
    }
  };
  if (CELL == MMDA_CELL_LSTM) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int t0 = dir ? 0 : T - 1;
      c_keep[r] = ldf(rc, t0 < len_r[r] ? oc[r] + (unsigned)t0 * scc : OOB);
    }
  }
  load_raw(0);
  derive(0);
  load_raw(1);
  // exchange image per parity: [consumer tile nt][m-tile][producer tile][64 lanes] x 8 B
  const unsigned slot_b = (unsigned)xchg_slot(NC, Hp);
  // One region of RS bytes per (consumer tile, m-tile).  Two arrangements of the producers' 512-byte partials inside it:
  //   write-through form : [producer][lane] x 8 B          -- every 128-byte line is written whole by one wave's store
  //   XCD-local form     : [producer pair][lane][2] x 8 B  -- the consumer fetches two producers per 16-byte load (half the load
  //                        instructions of the gather; the 8-byte halves of a line come from two waves, which L2 merges)
  const unsigned RS = (unsigned)((nHT + 1) & ~1) * 512u;
  const unsigned img_b = (unsigned)(nHT * 2) * RS;
  const __amdgpu_buffer_rsrc_t xr = make_rsrc(Xb, slot_b + img_b);
  const unsigned gat_base = (unsigned)(ht * 2 + mt) * RS + (unsigned)lane * 8u;          // + producer * 512
  const unsigned pub_base = (unsigned)mt * RS + (unsigned)(hp * 64 + lane) * 8u;         // + consumer tile nt * pub_stride
  const unsigned gat_base2 = (unsigned)(ht * 2 + mt) * RS + (unsigned)lane * 16u;        // + producer pair * 1024
  const unsigned pub_base2 = (unsigned)mt * RS + (unsigned)(hp >> 1) * 1024u + (unsigned)lane * 16u + (unsigned)(hp & 1) * 8u;
  const unsigned pub_stride = 2u * RS;
  bool paired = false;                                  // arrangement of the image the NEXT gather reads (= what the last publish used)

  unsigned long long ph[8] = {0, 0, 0, 0, 0, 0, 0, 0}, last = 0;
#define STAMP(i) do { if (DBG && L.dbg && tid == 0) { unsigned long long now_ = __builtin_readcyclecounter(); ph[i] += now_ - last; last = now_; } } while (0)
  if (DBG && L.dbg && tid == 0) last = __builtin_readcyclecounter();
  bool alive = true;
  typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;
  float dgv[4][4];                                      // fp32 dG of the previous step, stored behind the next step's gather loads
  const __amdgpu_buffer_rsrc_t rg16 = make_rsrc(D.dg16, D.dg16 ? (unsigned)T * B * 2u * G4 * 2u : 0u);
  const bool has_dg16 = D16 == 2 ? (gm && D.dg16 != nullptr) : (D16 == 1);       // workgroup-uniform
  const bool f32_dg = D16 == 2 ? !(has_dg16 && D.dg16_only) : (D16 == 0);
  auto flush = [&](int ps) {
    const int t = dir ? ps : T - 1 - ps;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const unsigned o = inb[r] ? og[r] + (unsigned)t * sg : OOB;       // zero at padded positions too
      if (gm) {
        if (f32_dg) stf4(rg, o, f32x4{dgv[r][0], dgv[r][1], dgv[r][2], dgv[r][3]});
        if (has_dg16) {                                // the same four values rounded to bf16: 8 bytes at half the byte offset
          const u32x2 pk = {pack_bf16x2(dgv[r][0], dgv[r][1]), pack_bf16x2(dgv[r][2], dgv[r][3])};
          __builtin_amdgcn_raw_buffer_store_b64(pk, rg16, inb[r] ? (og[r] + (unsigned)t * sg) >> 1 : OOB, 0, STASH_AUX);
        }
      } else {
#pragma unroll
        for (int g = 0; g < 4; ++g) stf(rg, inb[r] ? o + g * H * 4u : OOB, dgv[r][g]);
      }
    }
  };
  bool fast = false;                                    // XCD-local hand-off in force (see xcc_announce)
  const unsigned xcc = my_xcc_id() ^ ((L.xcd_local == 3 && (ht & 1)) ? 8u : 0u);   // (3: test hook, odd tiles announce a wrong id)
  if (L.xcd_local && lane == 0) xcc_announce(my_flag, L.epoch_base, xcc);
  // One step of the walk.  FIRST (step 0: nothing to gather) and FM (hand-off form: 0 = the `fast` / `paired` variables -- steps 0 and
  // 1, before and while the placement is being checked --, 1 = XCD-local and paired for sure, 2 = write-through and unpaired for sure)
  // are compile-time tags: the steady-state steps carry no step-number or form branches (each one, taken or not, splits the wave's
  // instruction schedule; see the forward kernel).
  // ROLE (PAIR kernels; compile-time: the accumulators a wave keeps are static registers): 0 = even tile of a pair (keeps the even
  // consumer tiles), 1 = odd tile (keeps the odd ones), 2 = no partner (keeps everything; also every wave of a PAIR = 0 kernel)
  auto do_step = [&](int step, auto first_tag, auto fm_tag, auto role_tag) {
    constexpr bool FIRST = decltype(first_tag)::value;
    constexpr int FM = decltype(fm_tag)::value;
    constexpr int ROLE = decltype(role_tag)::value;
    constexpr int NGQ = PAIR ? NTM / 4 : NTM / 2;        // 16-byte gather loads (two producers each)
    constexpr int NGP = PAIR ? NTM / 2 : NTM;            // 8-byte gather loads (one producer each)
    const unsigned epoch = L.epoch_base + (unsigned)step + 1u;
    float dh_rec[4] = {0.f, 0.f, 0.f, 0.f};
    if (!FIRST) {
      const unsigned need = epoch - 1u;
      alive = poll_tiles(poll_flag, abort_w, lane < nHT, need);
      if (!alive) { if (lane == 0) st_flag(abort_w, 1u); return; }
      if (FM == 0 && L.xcd_local && step == 1) fast = xcc_all_local(poll_flag, lane < nHT, L.epoch_base, xcc);
      STAMP(0);
      const unsigned par = (need & 1u) * slot_b;
      if (FM == 0 ? paired : FM == 1) {                  // wave-uniform (compile-time in the steady state)
        u32x4 gq[NGQ];
#pragma unroll
        for (int q = 0; q < NGQ; ++q)
          gq[q] = __builtin_amdgcn_raw_buffer_load_b128(xr, gat_base2 + (2 * q < nP ? par + (unsigned)q * 1024u : FAR), 0, 16);
        flush(step - 1);
        load_raw(step + 1);                              // consumed by derive() at the end of this step
        STAMP(1);
#pragma unroll
        for (int q = 0; q < NGQ; ++q) {                  // same summation order as the unpaired form: producer 2q, then 2q + 1
          const bool two = 2 * q + 1 < nP;               // the upper half of an odd count's last pair was written by nobody
          const unsigned b0 = two ? gq[q][2] : 0u, b1 = two ? gq[q][3] : 0u;
          dh_rec[0] += __builtin_bit_cast(float, gq[q][0] << 16);
          dh_rec[1] += __builtin_bit_cast(float, gq[q][0] & 0xffff0000u);
          dh_rec[2] += __builtin_bit_cast(float, gq[q][1] << 16);
          dh_rec[3] += __builtin_bit_cast(float, gq[q][1] & 0xffff0000u);
          dh_rec[0] += __builtin_bit_cast(float, b0 << 16);
          dh_rec[1] += __builtin_bit_cast(float, b0 & 0xffff0000u);
          dh_rec[2] += __builtin_bit_cast(float, b1 << 16);
          dh_rec[3] += __builtin_bit_cast(float, b1 & 0xffff0000u);
        }
      } else {
        u32x2 gv[NGP];
#pragma unroll
        for (int p = 0; p < NGP; ++p)
          gv[p] = __builtin_amdgcn_raw_buffer_load_b64(xr, gat_base + (p < nP ? par + (unsigned)p * 512u : FAR), 0, 16);
        flush(step - 1);
        load_raw(step + 1);                              // consumed by derive() at the end of this step
        STAMP(1);
#pragma unroll
        for (int p = 0; p < NGP; ++p) {
          dh_rec[0] += __builtin_bit_cast(float, gv[p][0] << 16);
          dh_rec[1] += __builtin_bit_cast(float, gv[p][0] & 0xffff0000u);
          dh_rec[2] += __builtin_bit_cast(float, gv[p][1] << 16);
          dh_rec[3] += __builtin_bit_cast(float, gv[p][1] & 0xffff0000u);
        }
      }
    }
    if (DBG && L.dbg) { asm volatile("s_nop 0" :: "v"(dh_rec[0]), "v"(dh_rec[1]), "v"(dh_rec[2]), "v"(dh_rec[3])); STAMP(2); }
    // lane-local gate gradients of the own hidden units: linear in dh / dc with the factors derive() prepared
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float dh = dh_rec[r] + dv.dh[r];
      float dp[4];
      if (CELL == MMDA_CELL_GRU) {
        dh += dc[r];
        const float dpn = dh * dv.a[0][r];
        dp[0] = dpn * dv.a[1][r];
        dp[1] = dh * dv.a[2][r];
        dp[2] = dpn;
        dp[3] = dpn * dv.a[3][r];
        dc[r] = dh * dv.a[5][r];
      } else {
        const float dct = dc[r] + dh * dv.a[4][r];
        dp[0] = dct * dv.a[0][r];
        dp[1] = dct * dv.a[1][r];
        dp[2] = dct * dv.a[2][r];
        dp[3] = dh * dv.a[3][r];
        dc[r] = dct * dv.a[5][r];
      }
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        Tr[(fq * 4 + r) * 64 + g * 16 + fr] = f2bf(dp[g]);
        dgv[r][g] = dp[g];
      }
    }
    if (step + 1 < T) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");            // the dG tile is complete in the wave-private LDS block
      STAMP(3);
      // A fragments of the two k-steps (gate pairs): row fr, 8 consecutive k at 32 ks2 + 8 fq
      const bf16x8 a0 = *reinterpret_cast<const bf16x8*>(&Tr[fr * 64 + fq * 8]);
      const bf16x8 a1 = *reinterpret_cast<const bf16x8*>(&Tr[fr * 64 + 32 + fq * 8]);
      const unsigned par = (epoch & 1u) * slot_b;
      // All 2 x NTM MFMAs first, into accumulators of their own (left to itself the compiler reuses ONE accumulator and waits out
      // every dependent pair before it converts and stores: ~210 cycles per column tile instead of ~32), then convert + store.
      // Column tiles past nHT multiply zero fragments and store to the out-of-range offset.
      f32x4 accs[NTM];
#pragma unroll
      for (int nt = 0; nt < NTM; ++nt) accs[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, wreg[nt][0], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
#pragma unroll
      for (int nt = 0; nt < NTM; ++nt) accs[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, wreg[nt][1], accs[nt], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      if (PAIR && ROLE < 2) {
        // hand the partner the tiles IT keeps (consumer tiles of the other parity), take its half of mine: fp32, through LDS
#pragma unroll
        for (int j = 0; j < NTM / 2; ++j) xmine[j * 64] = accs[2 * j + (1 - ROLE)];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        if (lane == 0) lflag[wave] = epoch;
        bool got = false;
        for (unsigned spins = 0; spins < (SPIN_LIMIT << 2); ++spins) {
          if ((int)(lflag[wave ^ 2] - epoch) >= 0) { got = true; break; }
          __builtin_amdgcn_s_sleep(1);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        if (!got) { alive = false; if (lane == 0) st_flag(abort_w, 1u); return; }
#pragma unroll
        for (int j = 0; j < NTM / 2; ++j) accs[2 * j + ROLE] += xpart[j * 64];
      }
      // the tile-dependent part of the offset is wave-uniform (scalar select, one vector add); tiles past nHT go out of range
      const bool fst = FM == 0 ? fast : FM == 1;
      constexpr int NPUB = (PAIR && ROLE < 2) ? NTM / 2 : NTM;       // tiles this wave publishes: its parity's, or all
      if (fst) {
#pragma unroll
        for (int j = 0; j < NPUB; ++j) {
          constexpr int dummy = 0; (void)dummy;
          const int nt = (PAIR && ROLE < 2) ? 2 * j + ROLE : j;
          const f32x4 av = accs[(PAIR && ROLE < 2) ? 2 * j + ROLE : j];
          const u32x2 pk = {pack_bf16x2(av[0], av[1]), pack_bf16x2(av[2], av[3])};
          const unsigned so = nt < nHT ? par + (unsigned)nt * pub_stride : FAR;
          __builtin_amdgcn_raw_buffer_store_b64(pk, xr, pub_base2 + so, 0, 0);
        }
      } else {
#pragma unroll
        for (int j = 0; j < NPUB; ++j) {
          const int nt = (PAIR && ROLE < 2) ? 2 * j + ROLE : j;
          const f32x4 av = accs[(PAIR && ROLE < 2) ? 2 * j + ROLE : j];
          const u32x2 pk = {pack_bf16x2(av[0], av[1]), pack_bf16x2(av[2], av[3])};
          const unsigned so = nt < nHT ? par + (unsigned)nt * pub_stride : FAR;
          __builtin_amdgcn_raw_buffer_store_b64(pk, xr, pub_base + so, 0, 16);
        }
      }
      STAMP(4);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");               // this wave's stores have landed (in L2 / written through)
      STAMP(5);
      if (lane == 0) { if (fst) st_flag_plain(my_flag, epoch); else st_flag(my_flag, epoch); }
      paired = fst;
      __builtin_amdgcn_sched_barrier(0);                             // keep the folding behind the hand-off
      derive(step + 1);
    }
  };
  {
    int step = 0;
    typedef std::integral_constant<bool, true> TrueT;
    typedef std::integral_constant<bool, false> FalseT;
    typedef std::integral_constant<int, 0> FmVar;
    typedef std::integral_constant<int, 1> FmLocal;
    typedef std::integral_constant<int, 2> FmThrough;
    auto walk = [&](auto role_tag) {
      if (T > 0) { do_step(0, TrueT{}, FmVar{}, role_tag); step = 1; }
      if (T > 1 && alive) { do_step(1, FalseT{}, FmVar{}, role_tag); step = 2; }
      if (fast) { for (; step < T && alive; ++step) do_step(step, FalseT{}, FmLocal{}, role_tag); }
      else { for (; step < T && alive; ++step) do_step(step, FalseT{}, FmThrough{}, role_tag); }
    };
    if constexpr (PAIR != 0) {
      if (!has_partner) walk(std::integral_constant<int, 2>{});      // wave-uniform
      else if (ht & 1) walk(std::integral_constant<int, 1>{});
      else walk(std::integral_constant<int, 0>{});
    } else {
      walk(std::integral_constant<int, 2>{});
    }
    if (alive && T > 0) flush(T - 1);
  }
  if (DBG && L.dbg && tid == 0)
    for (int i = 0; i < 8; ++i) L.dbg[(size_t)role * 8 + i] = ph[i];
#undef STAMP
}

}  // namespace

Kernel wave_kernel(int id, bool bwd) {
  constexpr int LSTM = MMDA_CELL_LSTM, GRU = MMDA_CELL_GRU;
  Kernel f = nullptr, b = nullptr;
  switch (id) {
    case MMDA_LSTM_K_FWD_WAVE_GM_NOSTASH: f = lstm_fwd_wave_kernel<10, true, LSTM, false, 1>; break;
    case MMDA_LSTM_K_FWD_WAVE_GM: f = lstm_fwd_wave_kernel<10, true, LSTM, false, 0>; break;
    case MMDA_LSTM_K_FWD_WAVE: f = lstm_fwd_wave_kernel<10, false, LSTM, false>; break;
    case MMDA_LSTM_K_FWD_WAVE_GRU_GM: f = lstm_fwd_wave_kernel<10, true, GRU, false>; break;
    case MMDA_LSTM_K_FWD_WAVE_GRU: f = lstm_fwd_wave_kernel<10, false, GRU, false>; break;
    case MMDA_LSTM_K_BWD_WAVE_ABSENT_PAIR: b = lstm_bwd_wave_kernel<20, true, LSTM, false, 0, 1, 1>; break;
    case MMDA_LSTM_K_BWD_WAVE_ABSENT: b = lstm_bwd_wave_kernel<20, true, LSTM, false, 0, 1>; break;
    case MMDA_LSTM_K_BWD_WAVE_PRESENT_PAIR: b = lstm_bwd_wave_kernel<20, true, LSTM, false, 1, 1, 1>; break;
    case MMDA_LSTM_K_BWD_WAVE_PRESENT: b = lstm_bwd_wave_kernel<20, true, LSTM, false, 1, 1>; break;
    case MMDA_LSTM_K_BWD_WAVE_GM: b = lstm_bwd_wave_kernel<20, true, LSTM, false>; break;
    case MMDA_LSTM_K_BWD_WAVE: b = lstm_bwd_wave_kernel<20, false, LSTM, false>; break;
    case MMDA_LSTM_K_BWD_WAVE_GRU_GM: b = lstm_bwd_wave_kernel<20, true, GRU, false>; break;
    case MMDA_LSTM_K_BWD_WAVE_GRU: b = lstm_bwd_wave_kernel<20, false, GRU, false>; break;
    case MMDA_LSTM_K_STAMPED: f = lstm_fwd_wave_kernel<10, true, LSTM, true>; b = lstm_bwd_wave_kernel<20, true, LSTM, true>; break;
  }
  return bwd ? b : f;
}

}  // namespace mmda_resident
