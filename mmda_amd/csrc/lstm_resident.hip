// Resident recurrences, host side (lstm_resident.h): the launch plan (plan_resident: the single place that decides form, waves per
// block and chunking), the instance table and pick_instance, block placement, the C entry points that view a plan, and the launch
// itself.  No kernel lives here: lstm_barrier.hip, lstm_wave.hip and lstm_quad.hip hand theirs over by instance id.
#include "lstm_resident.h"
#include "dynamic_lds.h"

using namespace mmda_resident;

namespace {

constexpr int MAX_WG_PER_LAUNCH = 240;   // one block per CU (LDS > 80 KB each, or the whole-LDS reservation), all co-resident
// Measured (MOSEI shapes, 108 tiles per 32-sample group): 216 and 432 workgroups (B = 64, 128) beat the one-wave-per-tile kernels by
// 8 % and 6 % of the step, 864 (B = 256, 3.4 workgroups per CU) lose 3 % -- there the CUs' issue slots, not the hand-off, set the pace
// (sleeping longer between polls changes nothing).
constexpr int MAX_WG_QUAD = 512;
struct Plan { int TPW, NC; size_t lds_f, lds_b; bool ok; };
// the roundings of one hidden size: Hp = H in 16-wide hidden tiles (nHT of them), Kp = H in 32-deep k-steps (KS of them)
struct Geom { int Hp, Kp, KS, nHT; };

Geom geom_of(int H) {
  const int Hp = round_up(H, 16), Kp = round_up(H, 32);
  return {Hp, Kp, Kp / 32, Hp / 16};
}

// barrier form: hidden tiles per workgroup and workgroups per cluster such that both passes' LDS fits
Plan plan_for(int H) {
  Plan p{};
  const Geom g = geom_of(H);
  const size_t cap = 160 * 1024 - 1024;
  for (int t = 2; t >= 1; --t) {          // <= 2 hidden tiles per workgroup: every wave owns exactly one (m-tile, hidden tile)
    if (t > g.nHT && t > 1) continue;
    size_t lf = (size_t)t * 4 * g.KS * 1024 + (size_t)2 * GROUP * (g.Kp + 8) * 2 + 16;
    const int nc = ceil_div(g.nHT, t);
    size_t lb = (size_t)t * g.nHT * 2 * 1024 + (size_t)GROUP * (t * 64 + 8) * 2 + (size_t)GROUP * (g.Hp + 8) * 2 +
                (size_t)(nc > 1 ? nc - 1 : 1) * GROUP * t * 16 * 2 + 16;
    if (lf <= cap && lb <= cap) {
      p.TPW = t; p.NC = nc; p.lds_f = lf; p.lds_b = lb; p.ok = p.NC <= 64;
      break;
    }
  }
  return p;
}

}  // namespace

// ---------------------------------------------------------------------------------------------- host entry (used by lstm.hip)
extern "C" int64_t mmda_lstm_xchg_bytes(int H, int B) {
  if (H <= 0 || H > 512 || B <= 0) return MMDA_EINVAL;
  Plan p = plan_for(H);
  if (!p.ok) return 0;                      // no cluster plan: the streaming kernel is used, no exchange buffer needed
  return (int64_t)((xchg_bytes(ceil_div(B, GROUP), p.NC, geom_of(H).Hp) + 255) & ~(size_t)255);
}

static unsigned long long* g_dbg = nullptr;
// diagnostics only (tools/): device buffer of 8 x u64 per workgroup receiving the forward kernel's phase cycle sums
extern "C" int mmda_debug_set_lstm_stamps(void* device_buffer) { g_dbg = (unsigned long long*)device_buffer; return MMDA_OK; }

namespace {
// Barrier: lstm_{fwd,bwd}_cluster_kernel (W_hh in LDS, workgroup barriers around the exchange).  Wave: lstm_{fwd,bwd}_wave_kernel
// (W_hh fragments in registers, 1, 2 or 4 autonomous waves per block).  Quad: lstm_{fwd,bwd}_quad_kernel (four waves per tile).
enum class Form { Barrier, Wave, Quad };
// what a backward instance knows about mmda_lstm_desc.d_hseq at compile time
enum class DHseq { RunTime, Absent, Present };

// Everything that decides which kernel runs and how, for one mmda_lstm_fwd / mmda_lstm_bwd call.  What depends on the chunk of
// batch groups (L.g0 / L.ng, block placement, grid size, the whole-LDS reservation) is worked out per launch from this.
struct ResidentPlan {
  bool ok, bwd;                            // ok = false: not applicable, the streaming kernels run
  Form form;
  int n, ngt, wpb, threads;                // descriptors, 32-sample batch groups, waves per block (wave form; 4 otherwise), block size
  Geom geom[MAXD];
  Plan barrier[MAXD];
  int members[MAXD];                       // workgroups per cluster
  int wg_per_group, groups_per_launch;
  bool gru, gate_minor, no_stash, pair_bwd, stamped;
  DHseq dhseq;
  size_t lds;                              // dynamic LDS of a launch that does not reserve the CU's whole LDS
};

// every block of a quad launch must be resident at once: at most what the occupancy query grants per CU (registers, 32 KB of LDS)
int quad_block_cap(bool bwd) {
  auto per_cu = [](const void* f) {
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, f, 256, QUAD_LDS) != hipSuccess) { (void)hipGetLastError(); nb = 1; }
    return nb < 1 ? 1 : (nb > 4 ? 4 : nb);
  };
  static const int occ_f = std::min(per_cu(reinterpret_cast<const void*>(quad_kernel(MMDA_LSTM_K_FWD_QUAD, false))),
                                    per_cu(reinterpret_cast<const void*>(quad_kernel(MMDA_LSTM_K_FWD_QUAD_GRU, false))));
  static const int occ_b = std::min(per_cu(reinterpret_cast<const void*>(quad_kernel(MMDA_LSTM_K_BWD_QUAD, true))),
                                    per_cu(reinterpret_cast<const void*>(quad_kernel(MMDA_LSTM_K_BWD_QUAD_GRU, true))));
  return std::min(MAX_WG_QUAD, 240 * (bwd ? occ_b : occ_f));
}

// What a plan takes from outside the descriptors.  quad_cap: the most blocks a quad launch may hold -- QUAD_CAP_RUNTIME asks the
// runtime (quad_block_cap: a launch, and the plan view on a device), QUAD_CAP_NEVER (the two probes) makes no HIP runtime call and
// reports Quad as Wave: neither plan.ok nor "not the barrier form" depends on the difference.  no_quad: MMDA_LSTM_NO_QUAD.
constexpr int QUAD_CAP_RUNTIME = 0, QUAD_CAP_NEVER = -1;
struct PlanSwitches { bool no_quad; int quad_cap; };

// The single place that decides.
ResidentPlan plan_resident(int n, const mmda_lstm_desc* descs, int B, int T, bool bwd, const PlanSwitches& sw) {
  ResidentPlan P{};
  if (n > MAXD || n <= 0) return P;
  P.n = n; P.bwd = bwd; P.ngt = ceil_div(B, GROUP);
  P.gru = descs[0].cell == MMDA_CELL_GRU;
  P.gate_minor = descs[0].gate_minor != 0;
  // Wave form <=> every H <= 320: W_hh's k-steps (<= 10) then fit the register-resident form.  Such descriptors always fit one
  // launch at four waves per block: <= MAXD * 2 * ceil(2 * 20 / 4) = 80 of the 240 workgroups.  (Beyond 320 hidden units the
  // barrier-synchronised kernels run instead; where both fit, they measured slower.)
  bool wave = P.no_stash = true;
  for (int i = 0; i < n; ++i) {
    P.geom[i] = geom_of(descs[i].H);
    wave = wave && P.geom[i].KS <= 10;
    P.no_stash = P.no_stash && descs[i].forward_only;
  }
  // the checks that decide whether the resident-weights kernels can run these descriptors
  size_t lds_barrier = 0; int wg_barrier = 0;
  for (int i = 0; i < n; ++i) {
    const mmda_lstm_desc& d = descs[i];
    if (!d.xchg || d.cell != descs[0].cell || d.gate_minor != descs[0].gate_minor) return P;
    // the GRU cell exists in the wave-autonomous kernels only (and in the streaming kernels of lstm.hip)
    if (d.cell != MMDA_CELL_LSTM && !wave) return P;
    if (bwd && (!d.wpack_c[0] || !d.wpack_c[1])) return P;
    P.barrier[i] = plan_for(d.H);
    if (!P.barrier[i].ok) return P;
    // buffer descriptors address 32-bit byte offsets: every per-step tensor must stay below 4 GiB
    if ((double)T * B * 2.0 * 4.0 * d.H * 4.0 >= 4.0e9) return P;
    lds_barrier = std::max(lds_barrier, bwd ? P.barrier[i].lds_b : P.barrier[i].lds_f);
    wg_barrier += 2 * P.barrier[i].NC;
  }
  if (wg_barrier > MAX_WG_PER_LAUNCH) return P;
  P.ok = true;

  // Wave form: blocks hold 1, 2 or 4 waves (one (hidden tile, m-tile) each): the fewest waves per block with which ALL ngt batch
  // groups still fit one launch, because the waves of a block share the CU's address unit and the per-step memory instructions are
  // what they queue on.  (B = 256: eight groups, 864 waves = 240 four-wave blocks, one wave per SIMD.)  The groups are independent
  // chains, and a second launch for the groups that did not fit costs a whole extra walk of the sequence, where more waves per CU
  // cost a fraction of a step.  (Fitting one group only measured slower.)
  auto wave_wgs = [&](int w) { int t = 0; for (int i = 0; i < n; ++i) t += 2 * ceil_div(2 * P.geom[i].nHT, w); return t; };
  P.wpb = wave ? 1 : 4;
  while (P.wpb < 4 && wave_wgs(P.wpb) * P.ngt > MAX_WG_PER_LAUNCH) P.wpb *= 2;
  // Four waves per tile: gate-minor layout, every group's tiles in one launch at one workgroup per tile (the quad kernels' own
  // limits, 12 k-steps and 20 hidden tiles, are wider than the wave form's).  MMDA_LSTM_NO_QUAD: ablation (the one-wave-per-tile
  // kernels).
  const bool quad = sw.quad_cap != QUAD_CAP_NEVER && wave && P.gate_minor && !sw.no_quad && g_dbg == nullptr &&
                    wave_wgs(1) * P.ngt <= (sw.quad_cap > 0 ? sw.quad_cap : quad_block_cap(bwd));
  if (quad) P.wpb = 1;
  P.form = quad ? Form::Quad : (wave ? Form::Wave : Form::Barrier);
  for (int i = 0; i < n; ++i) {
    P.members[i] = wave ? ceil_div(2 * P.geom[i].nHT, P.wpb) : P.barrier[i].NC;
    P.wg_per_group += 2 * P.members[i];
  }
  // (the max: H <= 0 reaches the probes, never a launch)
  P.groups_per_launch = quad ? P.ngt : MAX_WG_PER_LAUNCH / std::max(P.wg_per_group, 1);
  P.threads = (wave && !quad) ? 64 * P.wpb : 256;

  // the cycle stamps of tools/diag_lstm_phases.py live in a kernel instance of their own (gate-minor LSTM only): even a never-taken
  // branch per phase costs the production kernels scheduling freedom
  P.stamped = g_dbg != nullptr && wave && !P.gru && P.gate_minor;
  // backward, four waves per block (large batches): the two waves of an m-tile pre-reduce their partial dh tiles in LDS and publish
  // one partial per producer PAIR (lstm_bwd_wave_kernel<..., PAIR = 1>): 4 x 2 KB + 4 x 10 KB + the epoch words.
  P.pair_bwd = bwd && wave && !quad && P.wpb == 4 && P.gate_minor && !P.gru && g_dbg == nullptr;
  // backward, production form (gate-minor, dG as bf16 only): instances that know at compile time whether d_hseq exists (layer 1:
  // present, layer 2: absent); anything else takes the instance that decides at run time
  P.dhseq = DHseq::RunTime;
  if (bwd && wave && P.gate_minor) {
    bool all16 = true, any_dh = false, all_dh = true;
    for (int i = 0; i < n; ++i) {
      all16 = all16 && descs[i].dg_bf16 != nullptr && descs[i].dg_bf16_only;
      any_dh = any_dh || descs[i].d_hseq != nullptr;
      all_dh = all_dh && descs[i].d_hseq != nullptr;
    }
    if (all16 && (all_dh || !any_dh)) P.dhseq = all_dh ? DHseq::Present : DHseq::Absent;
  }
  const size_t lds_wave = P.pair_bwd ? 4 * 2048 + 4 * 10240 + 64 : 4 * 2048;      // 2 KB per wave (+ the pair pre-reduction)
  P.lds = quad ? (size_t)QUAD_LDS : (wave ? lds_wave : lds_barrier);
  return P;
}

// The instance table.  One name per MMDA_LSTM_K_* (include/mmda_hip.h), in the enum's order: by form (Barrier, Wave, Quad), then
// pass (forward, backward), then specialisation; the stamped debug instance is one id with a kernel per pass.  The functions live
// in the form's own file: barrier_kernel, wave_kernel and quad_kernel each know their ids and answer nullptr to the others'.
const char* instance_name(int id) {
  static const char* const names[MMDA_LSTM_K_COUNT] = {
      "lstm_fwd_cluster_kernel<10,true>", "lstm_fwd_cluster_kernel<10,false>", "lstm_bwd_cluster_kernel<true>", "lstm_bwd_cluster_kernel<false>",
      "lstm_fwd_wave_kernel<10,true,LSTM,false,1>", "lstm_fwd_wave_kernel<10,true,LSTM,false,0>", "lstm_fwd_wave_kernel<10,false,LSTM,false>",
      "lstm_fwd_wave_kernel<10,true,GRU,false>", "lstm_fwd_wave_kernel<10,false,GRU,false>",
      "lstm_bwd_wave_kernel<20,true,LSTM,false,0,1,1>", "lstm_bwd_wave_kernel<20,true,LSTM,false,0,1>",
      "lstm_bwd_wave_kernel<20,true,LSTM,false,1,1,1>", "lstm_bwd_wave_kernel<20,true,LSTM,false,1,1>",
      "lstm_bwd_wave_kernel<20,true,LSTM,false>", "lstm_bwd_wave_kernel<20,false,LSTM,false>",
      "lstm_bwd_wave_kernel<20,true,GRU,false>", "lstm_bwd_wave_kernel<20,false,GRU,false>",
      "stamped debug instance",
      "lstm_fwd_quad_kernel<LSTM,1>", "lstm_fwd_quad_kernel<LSTM,0>", "lstm_fwd_quad_kernel<GRU,1>", "lstm_fwd_quad_kernel<GRU,0>",
      "lstm_bwd_quad_kernel<LSTM,1,1>", "lstm_bwd_quad_kernel<LSTM,0,1>", "lstm_bwd_quad_kernel<LSTM,2,2>", "lstm_bwd_quad_kernel<GRU,2,2>",
  };
  return names[id];
}
Kernel instance_kernel(int id, bool bwd) {
  for (auto ask : {barrier_kernel, wave_kernel, quad_kernel})
    if (Kernel k = ask(id, bwd)) return k;
  return nullptr;
}

// Which instance a plan runs (no function is named here: the view of a plan needs the answer without a launch).
int pick_instance(const ResidentPlan& P) {
  const bool gm = P.gate_minor, wave = P.form == Form::Wave;
  if (P.form == Form::Quad) {              // gate-minor only
    if (P.bwd) {
      if (P.gru) return MMDA_LSTM_K_BWD_QUAD_GRU;
      if (P.dhseq == DHseq::Present) return MMDA_LSTM_K_BWD_QUAD_PRESENT;
      if (P.dhseq == DHseq::Absent) return MMDA_LSTM_K_BWD_QUAD_ABSENT;
      return MMDA_LSTM_K_BWD_QUAD;
    }
    if (P.gru) return P.no_stash ? MMDA_LSTM_K_FWD_QUAD_GRU_NOSTASH : MMDA_LSTM_K_FWD_QUAD_GRU;
    return P.no_stash ? MMDA_LSTM_K_FWD_QUAD_NOSTASH : MMDA_LSTM_K_FWD_QUAD;
  }
  // wave form, stamped: a debug instance of its own (see plan_resident)
  if (P.stamped) return MMDA_LSTM_K_STAMPED;
  if (P.gru) {                             // wave form (plan_resident admits the GRU cell to no other)
    if (P.bwd) return gm ? MMDA_LSTM_K_BWD_WAVE_GRU_GM : MMDA_LSTM_K_BWD_WAVE_GRU;
    return gm ? MMDA_LSTM_K_FWD_WAVE_GRU_GM : MMDA_LSTM_K_FWD_WAVE_GRU;
  }
  if (P.bwd && wave) {
    // gate-minor with dG as bf16 only: d_hseq is known at compile time; pairing only at four waves per block (plan_resident)
    if (P.dhseq == DHseq::Absent) return P.pair_bwd ? MMDA_LSTM_K_BWD_WAVE_ABSENT_PAIR : MMDA_LSTM_K_BWD_WAVE_ABSENT;
    if (P.dhseq == DHseq::Present) return P.pair_bwd ? MMDA_LSTM_K_BWD_WAVE_PRESENT_PAIR : MMDA_LSTM_K_BWD_WAVE_PRESENT;
    return gm ? MMDA_LSTM_K_BWD_WAVE_GM : MMDA_LSTM_K_BWD_WAVE;
  }
  if (P.bwd) return gm ? MMDA_LSTM_K_BWD_BARRIER_GM : MMDA_LSTM_K_BWD_BARRIER;      // barrier form
  if (wave) {
    if (gm) return P.no_stash ? MMDA_LSTM_K_FWD_WAVE_GM_NOSTASH : MMDA_LSTM_K_FWD_WAVE_GM;
    return MMDA_LSTM_K_FWD_WAVE;
  }
  return gm ? MMDA_LSTM_K_FWD_BARRIER_GM : MMDA_LSTM_K_FWD_BARRIER;   // barrier form
}

Kernel pick_kernel(const ResidentPlan& P) { return instance_kernel(pick_instance(P), P.bwd); }

// Placement (speed only): blocks b and b + 8 are dealt to the same XCD, so the members of one cluster (first role, members; its
// roles are first, first + stride, ...) get block ids that are equal mod 8; clusters go, largest first, to the XCD with the
// fewest members so far.  Returns false, with the identity map, when some XCD's per_xcd block slots do not suffice.
bool place_blocks(std::vector<std::pair<int, int>>& clusters, int stride, int per_xcd, int wg, short* blk2role, int* grid_blocks) {
  std::stable_sort(clusters.begin(), clusters.end(), [](const std::pair<int, int>& a, const std::pair<int, int>& b) { return a.second > b.second; });
  for (int b = 0; b < MAXB; ++b) blk2role[b] = -1;
  int used[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  int max_slots = 0;
  bool fits = wg <= 8 * per_xcd;
  for (size_t c = 0; fits && c < clusters.size(); ++c) {
    int x = 0;
    for (int k = 1; k < 8; ++k) if (used[k] < used[x]) x = k;
    fits = used[x] + clusters[c].second <= per_xcd;
    for (int j = 0; fits && j < clusters[c].second; ++j) blk2role[(used[x] + j) * 8 + x] = (short)(clusters[c].first + j * stride);
    used[x] += clusters[c].second;
    max_slots = std::max(max_slots, used[x]);
  }
  *grid_blocks = fits ? 8 * max_slots : wg;
  if (!fits) for (int b = 0; b < MAXB; ++b) blk2role[b] = (short)(b < wg ? b : -1);
  return fits;
}

}  // namespace

extern "C" int mmda_lstm_resident_applicable(int mode, int n, const mmda_lstm_desc* descs, int B, int T, int backward) {
  if (mode != MMDA_BF16 || !descs || B <= 0 || T <= 0) return 0;
  return plan_resident(n, descs, B, T, backward != 0, {false, QUAD_CAP_NEVER}).ok ? 1 : 0;
}

extern "C" int mmda_lstm_bwd_emits_dg_bf16(int mode, int n, const mmda_lstm_desc* descs, int B, int T) {
  // the wave-autonomous backward kernels with the gate-minor layout (one layout for all descriptors of a plan) are the ones that
  // write mmda_lstm_desc.dg_bf16
  if (mode != MMDA_BF16 || !descs || B <= 0 || T <= 0) return 0;
  const ResidentPlan P = plan_resident(n, descs, B, T, true, {false, QUAD_CAP_NEVER});
  return (P.ok && P.form != Form::Barrier && P.gate_minor) ? 1 : 0;
}

extern "C" int mmda_lstm_plan_describe(int n, const mmda_lstm_desc* descs, int B, int T, int backward, const int switches[2],
                                       mmda_lstm_plan* plan) {
  if (!descs || !plan || B <= 0 || T <= 0) return MMDA_EINVAL;
  *plan = mmda_lstm_plan{};
  plan->kernel = -1;
  for (int i = 0; i < n && i < MAXD; ++i)
    if (descs[i].H <= 0 || descs[i].H > 512) return MMDA_OK;           // mmda_lstm_fwd / bwd reject these before any plan is made
  const PlanSwitches sw = {switches && switches[0] != 0, (switches && switches[1] > 0) ? switches[1] : QUAD_CAP_RUNTIME};
  const ResidentPlan P = plan_resident(n, descs, B, T, backward != 0, sw);
  if (!P.ok) return MMDA_OK;
  plan->ok = 1;
  plan->form = P.form == Form::Quad ? MMDA_LSTM_FORM_QUAD : (P.form == Form::Wave ? MMDA_LSTM_FORM_WAVE : MMDA_LSTM_FORM_BARRIER);
  plan->wpb = P.wpb;
  plan->groups = P.ngt;
  plan->groups_per_launch = std::min(P.groups_per_launch, P.ngt);
  plan->launches = ceil_div(P.ngt, P.groups_per_launch);
  plan->wg_per_group = P.wg_per_group;
  for (int i = 0; i < n; ++i) plan->wg_per_desc[i] = 2 * P.members[i];
  plan->gru = P.gru; plan->gate_minor = P.gate_minor; plan->no_stash = P.no_stash;
  plan->dhseq = P.dhseq == DHseq::Present ? MMDA_LSTM_DHSEQ_PRESENT : (P.dhseq == DHseq::Absent ? MMDA_LSTM_DHSEQ_ABSENT : MMDA_LSTM_DHSEQ_RUNTIME);
  plan->kernel = pick_instance(P);
  // ResidentPlan.pair_bwd sizes the LDS of every gate-minor LSTM backward at four waves per block; only these two instances pair
  plan->pair = (plan->kernel == MMDA_LSTM_K_BWD_WAVE_ABSENT_PAIR || plan->kernel == MMDA_LSTM_K_BWD_WAVE_PRESENT_PAIR) ? 1 : 0;
  return MMDA_OK;
}

extern "C" const char* mmda_lstm_kernel_name(int kernel) {
  return (kernel >= 0 && kernel < MMDA_LSTM_K_COUNT) ? instance_name(kernel) : nullptr;
}

// returns MMDA_OK and sets *used = 1 when the cluster kernels ran; *used = 0 means "not applicable, use the streaming path"
int mmda_lstm_cluster_launch(int n, const mmda_lstm_desc* descs, int B, int T, const int32_t* lengths, void* stream, bool bwd,
                             int* used) {
  *used = 0;
  static const bool no_quad = mmda_env_set("MMDA_LSTM_NO_QUAD");
  const ResidentPlan P = plan_resident(n, descs, B, T, bwd, {no_quad, QUAD_CAP_RUNTIME});
  if (!P.ok) return MMDA_OK;
  const bool wave = P.form != Form::Barrier, quad = P.form == Form::Quad;
  const Kernel kernel = pick_kernel(P);
  if (!kernel) {                             // an instance id without a function for this pass must never reach the runtime
    mmda_set_error(bwd ? "mmda_lstm_bwd(cluster): no kernel" : "mmda_lstm_fwd(cluster): no kernel", hipErrorInvalidDeviceFunction);
    return MMDA_ELAUNCH;
  }
  static const int xcd_env = mmda_env_int("MMDA_XCD_LOCAL", 1);      // 0: ablation (always write through); 3: test hook
  for (int g0 = 0; g0 < P.ngt; g0 += P.groups_per_launch) {
    CLaunch L;
    L.n = n; L.B = B; L.T = T; L.g0 = g0; L.ng = std::min(P.ngt - g0, P.groups_per_launch);
    L.lengths = lengths; L.epoch_base = descs[0].epoch_base; L.dbg = g_dbg;
    L.gate_minor = P.gate_minor ? 1 : 0;
    L.wpb = P.wpb;
    L.no_stash = P.no_stash ? 1 : 0;
    int wg = 0;
    for (int i = 0; i < MAXD; ++i) {
      const int k = i < n ? i : 0;
      const mmda_lstm_desc& d = descs[k];
      const Geom& g = P.geom[k];
      CDesc& c = L.d[i];
      c.H = d.H; c.Hp = g.Hp; c.Kp = g.Kp; c.KS = g.KS; c.KSB = 4 * g.Hp / 32; c.nHT = g.nHT;
      c.TPW = P.barrier[k].TPW; c.NC = P.barrier[k].NC; c.NCw = P.members[k];
      c.gates = d.gates; c.cstash = d.cstash; c.hseq = d.hseq; c.wpack[0] = d.wpack[0]; c.wpack[1] = d.wpack[1];
      c.wpack_c[0] = d.wpack_c[0]; c.wpack_c[1] = d.wpack_c[1];
      c.utt = d.utt; c.layer = d.layer; c.d_hseq = d.d_hseq; c.xchg = (unsigned char*)d.xchg;
      c.dg16 = (bwd && wave && d.gate_minor) ? d.dg_bf16 : nullptr;
      c.dg16_only = (c.dg16 && d.dg_bf16_only) ? 1 : 0;
      c.wg_begin = wg;
      if (i < n) wg += 2 * L.ng * P.members[i];
    }
    // (first role, members).  Wave form with one wave per block: a wave exchanges data only with the waves of its own m-tile
    // (roles first + mt, first + mt + 2, ...), so each m-tile is a cluster of its own (19 blocks for text: fits an XCD's 32 CUs).
    const bool by_mt = wave && P.wpb == 1;
    std::vector<std::pair<int, int>> clusters;
    for (int i = 0; i < n; ++i)
      for (int c2 = 0; c2 < 2 * L.ng; ++c2) {
        const int first = L.d[i].wg_begin + c2 * P.members[i];
        if (by_mt) { clusters.push_back({first, P.members[i] / 2}); clusters.push_back({first + 1, P.members[i] / 2}); }
        else clusters.push_back({first, P.members[i]});
      }
    int grid_blocks = 0;
    const bool placed = place_blocks(clusters, by_mt ? 2 : 1, quad ? 32 * 4 : 32, wg, L.blk2role, &grid_blocks);
    // only the wave kernels verify the placement (per m-tile: every wave reads the XCC ids of all hidden tiles of its m-tile)
    // before they rely on it; the barrier-form kernels always write through
    L.xcd_local = (placed && wave) ? xcd_env : 0;
    // With one wave per block the kernel asks for the CU's whole LDS instead of what it needs: that keeps every LDS-using
    // workgroup of a concurrent kernel (weight-gradient GEMMs and conversions on the side stream) off the ~110 CUs that host a
    // recurrent wave, and leaves them the other ~145.
    // Only while the launch leaves a good part of the chip free (<= 160 blocks): every block then needs a CU of its own, and the
    // members of a cluster must all be resident at once -- a launch that wants most of the 256 CUs keeps the small allocation, so
    // that its blocks can share CUs if something else (another process on the GPU) holds some.
    const bool reserve = P.wpb == 1 && grid_blocks <= 160;
    const size_t lds_launch = reserve ? (size_t)160 * 1024 : P.lds;
    ensure_dynamic_lds(kernel, lds_launch);
    hipLaunchKernelGGL(kernel, dim3(grid_blocks), dim3(P.threads), lds_launch, (hipStream_t)stream, L);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { mmda_set_error(bwd ? "mmda_lstm_bwd(cluster)" : "mmda_lstm_fwd(cluster)", e); return MMDA_ELAUNCH; }
  }
  *used = 1;
  return MMDA_OK;
}
