// select.hpp -- the policy of the library: which kernel family, which ordering, which register instance and which LDS shape a sparsity
// pattern and batch size get (select_kernel), and every MPCQP_* environment switch that can bend it (Knobs).
//
// Pure C++ on top of plan.hpp (no HIP, same rule as there), so that the rule is testable without a GPU: tests/test_select.py runs it through
// tests/support/plan_interp.cpp against tests/golden/selection_grid.json.  mpcqp.hip applies the result: it uploads the chosen plans, looks the
// kernel instances up in the table (kernel_table.hpp) and asks the device for what only the device knows (resident workgroups).
#pragma once
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "plan.hpp"

namespace mpcqp {

// register-resident blocks per wave of the four-wave on-chip instance: inverse diagonal blocks (positions per wave) and hub blocks
constexpr int OC_NG = 5, OC_NH = 3;
// Long chains (more than 20 chain blocks: quadrotor N > 20, cart-pole N > 60): eight waves per QP, one workgroup per CU -- the whole LDS and
// 8 x 256 VGPRs for one factor.  Two instances: up to 32 chain blocks with every hub block in registers (cart-pole N = 100: 62 KB of chain
// blocks + 36 KB of vectors in LDS), and up to 56 with seven positions per wave, G_p and every hub block (both orientations) in registers --
// 168 resident VGPRs -- and only the chain blocks and the hub's inverse in LDS (quadrotor N = 50: 50 blocks = 100 KB + 57 KB of vectors and
// tables = 159,880 B).  (Measured against <NG 7, NH 5> with z, y in the slab, 157,832 B and 136 resident VGPRs: 35.5 against 35.9 ms and an
// eighth less HBM traffic -- the slab vectors cost more than the extra spills.)
struct Oc8Inst { int ng, nh; bool zyg; };
constexpr Oc8Inst OC8_INST[2] = {{4, 4, false}, {7, 7, false}};
constexpr long OC_LDS_MAX = 80 * 1024;      // four-wave on-chip instances: two workgroups per CU
constexpr long OC8_LDS_MAX = 160 * 1024;    // eight-wave ones: one (OC8_INST)
constexpr int OC8_MAX_CHAIN = 64;           // (oc_ldl keeps the chain's block ids one per lane)
constexpr long LDS_MAX = 160 * 1024;        // LDS of a CU

constexpr int SEL_ERR_ARG = 1, SEL_ERR_LIMIT = 5;      // = MPCQP_ERR_ARG, MPCQP_ERR_LIMIT of include/mpcqp.h (mpcqp.hip asserts it)

// Every MPCQP_* environment switch the library reads.  A handle reads them once, at create (from_env), and keeps them: changing the environment
// between create and solve changes nothing for that handle.  "set" = present in the environment with any value, unless a value is named.
struct Knobs {
  bool variant_named = false; std::string variant;   // MPCQP_VARIANT=stream|res1|res2|res4|res8|gres4|gres2|oc4|oc8: the family instead of the rule's choice (every kernel; ERR_LIMIT where it does not take the size)
  bool autotune = false;      // MPCQP_AUTOTUNE=1: mpcqp_create measures the families like mpcqp_create_tuned (not when MPCQP_VARIANT is set)
  bool verbose = false;       // MPCQP_VERBOSE: the set-up kernel's launch shape on stderr at create (two-kernel on-chip form)
  bool no_lpt = false;        // MPCQP_NO_LPT: no longest-first dispatch hint from the previous solve's iteration counts (every kernel)
  // ---- the rule
  bool no_twist = false;      // MPCQP_NO_TWIST: the stage chain eliminated from one end only (multi-wave kernels; the on-chip orders need the twist)
  bool no_oc = false;         // MPCQP_NO_OC: the rule never takes the on-chip mode (four- and eight-wave)
  bool no_oc8 = false;        // MPCQP_NO_OC8: long chains keep the global-block kernels instead of the eight-wave on-chip instances
  bool no_res2 = false;       // MPCQP_NO_RES2: the rule never takes two waves per QP (LDS-resident and global-block)
  bool no_dissect = false;    // MPCQP_NO_DISSECT: no dissected order (several twisted pairs): on-chip instances with one pair of chains only
  bool no_padtwist = false;   // MPCQP_NO_PADTWIST: four-wave on-chip mode without the padded twist (cart-pole N=22, 25 fall to other kernels)
  bool oc_mono = false;       // MPCQP_OC_MONO: the on-chip mode as one kernel instead of set-up + iteration (A/B runs; no hub-less eight-wave, no two-pair instance)
  bool oc_pad4 = false;       // MPCQP_OC_PAD4: four-wave on-chip mode keeps ELL widths in multiples of 4 instead of this instance's 8 slots in flight
  // ---- instances of a family
  bool no_zyg = false;        // MPCQP_NO_ZYG: four-wave global-block kernel keeps z, y in LDS on long horizons
  bool gb_occ2 = false;       // MPCQP_GB_OCC2: four-wave global-block kernel always in its 256-VGPR instance
  bool gb_occ3 = false;       // MPCQP_GB_OCC3: ... in its 168-VGPR instance below 40 KiB of LDS too
  bool no_res1x = false;      // MPCQP_NO_RES1X: one-wave kernel never in its 128-VGPR instance
  bool no_res3 = false;       // MPCQP_NO_RES3: LDS-resident four-wave kernel never in its 128- / 168-VGPR instances
  bool pd4 = false;           // MPCQP_PD4: streaming kernel with 4 blocks in flight whatever its LDS footprint
  long lds_min = 0;           // MPCQP_LDS_MIN=<bytes>: experiment, LDS request of the resident kernels padded up to limit workgroups per CU
  // ---- opt-in experiments of the on-chip mode (each measured slower: see the function that applies it)
  int tiles = 0;              // MPCQP_TILES=1: dense tiles of A on the matrix cores, single-kernel form (2); any other value (1) only keeps the two-pair instance away
  int vtiles = 0;             // MPCQP_VTILES=1: dense tiles of A on the vector ALUs, two-kernel form (2); any other value (1) as above
  int doubles = -1;           // MPCQP_DOUBLES=<n>: up to n double stages of the solve where LDS has room (-1: not set)
  bool late = false;          // MPCQP_LATE: single-kernel four-wave on-chip instance computes the late rows of the right-hand side behind a ticket
  // ---- two-kernel on-chip form
  int resume_rounds = 1;      // MPCQP_RESUME_ROUNDS=<0..8>: {re-factorisation, iteration} pairs queued behind a solve before the last pair
  bool no_ix16 = false;       // MPCQP_NO_IX16: set-up kernel without 16-bit index tables in LDS
  bool no_ruiz_regs = false;  // MPCQP_NO_RUIZ_REGS=1: set-up kernel's Ruiz passes reload their fixed operands (indices, P's values) every pass instead of keeping them in registers
  bool no_t_lds = false;      // MPCQP_NO_T_LDS=1: set-up kernel's assembly takes its T tiles through the slab instead of LDS, part by part (plan.hpp build_t_lds_plan)
  bool no_sing_list = false;  // MPCQP_NO_SING_LIST=1: set-up kernel's diagonal term walks all of A' for its flagged entries instead of reading their list (plan.hpp build_sing_list)
  bool no_setup_batch = false; // MPCQP_NO_SETUP_BATCH=1: set-up kernel's load and write-out phases one round trip at a time, as before DESIGN.md 3.13 (no batched stages, q through the slab, A' from the caller's array)
  long setup_cap = LONG_MIN;  // MPCQP_SETUP_CAP=<bytes>: LDS the set-up kernel's shape is fitted to, instead of a half or a third of a CU (LONG_MIN: not set)
  bool no_abalance = false;   // MPCQP_NO_ABALANCE: eight-wave iteration kernel takes A's row chunks round-robin instead of balanced by load batches
  bool no_touch = false;      // MPCQP_NO_TOUCH: no L2 touch by the idle waves during the backward chains (on-chip kernels)
  bool touch4 = false;        // MPCQP_TOUCH4: the touch back on for the four-wave instances of the two-kernel form
  bool touch8 = false;        // MPCQP_TOUCH8: ... for the eight-wave instances
  // ---- every solve
  bool no_remap = false;      // MPCQP_NO_REMAP: workgroup b solves instance b even with a dispatch hint (resident kernels)
  int pipe_streams = 2;       // MPCQP_PIPE_STREAMS=<1..8>: compute streams of mpcqp_solve_host

  static Knobs from_env() {
    auto set = [](const char *name) { return getenv(name) != nullptr; };
    auto one = [](const char *name) { const char *e = getenv(name); return !e ? 0 : e[0] == '1' ? 2 : 1; };
    Knobs k;
    if (const char *e = getenv("MPCQP_VARIANT")) { k.variant_named = true; k.variant = e; }
    k.autotune = one("MPCQP_AUTOTUNE") == 2;
    k.verbose = set("MPCQP_VERBOSE");
    k.no_lpt = set("MPCQP_NO_LPT");
    k.no_twist = set("MPCQP_NO_TWIST");
    k.no_oc = set("MPCQP_NO_OC");
    k.no_oc8 = set("MPCQP_NO_OC8");
    k.no_res2 = set("MPCQP_NO_RES2");
    k.no_dissect = set("MPCQP_NO_DISSECT");
    k.no_padtwist = set("MPCQP_NO_PADTWIST");
    k.oc_mono = set("MPCQP_OC_MONO");
    k.oc_pad4 = set("MPCQP_OC_PAD4");
    k.no_zyg = set("MPCQP_NO_ZYG");
    k.gb_occ2 = set("MPCQP_GB_OCC2");
    k.gb_occ3 = set("MPCQP_GB_OCC3");
    k.no_res1x = set("MPCQP_NO_RES1X");
    k.no_res3 = set("MPCQP_NO_RES3");
    k.pd4 = set("MPCQP_PD4");
    if (const char *e = getenv("MPCQP_LDS_MIN")) k.lds_min = atol(e);
    k.tiles = one("MPCQP_TILES");
    k.vtiles = one("MPCQP_VTILES");
    if (const char *e = getenv("MPCQP_DOUBLES")) k.doubles = std::max(0, atoi(e));
    k.late = set("MPCQP_LATE");
    if (const char *e = getenv("MPCQP_RESUME_ROUNDS")) k.resume_rounds = std::max(0, std::min(atoi(e), 8));
    k.no_ix16 = set("MPCQP_NO_IX16");
    k.no_ruiz_regs = one("MPCQP_NO_RUIZ_REGS") == 2;
    k.no_t_lds = one("MPCQP_NO_T_LDS") == 2;
    k.no_sing_list = one("MPCQP_NO_SING_LIST") == 2;
    k.no_setup_batch = one("MPCQP_NO_SETUP_BATCH") == 2;
    if (const char *e = getenv("MPCQP_SETUP_CAP")) k.setup_cap = atol(e);
    k.no_abalance = set("MPCQP_NO_ABALANCE");
    k.no_touch = set("MPCQP_NO_TOUCH");
    k.touch4 = set("MPCQP_TOUCH4");
    k.touch8 = set("MPCQP_TOUCH8");
    k.no_remap = set("MPCQP_NO_REMAP");
    if (const char *e = getenv("MPCQP_PIPE_STREAMS")) k.pipe_streams = std::max(1, std::min(atoi(e), 8));
    return k;
  }
};

// The set-up kernel's own launch shape in the two-kernel on-chip form.  Nothing of the factor is resident while it runs, so it does not need the
// iteration kernel's LDS (the block slots) or its eight waves: four-wave workgroups (oc_ldl's chain waves and helpers are four in any case) with an
// LDS request of their own let two or three QPs share a CU where the iteration kernel has one.  (Single-kernel form: the iteration's own shape.)
struct SetupShape {
  int nw = 0; long lds = 0, stage = 0;
  int a_lds = 0, p_lds = 0, ix16 = 0, zpad = 0, ixo_a = 0, ixo_p = 0;
  long vecs = 0, tabw = 0;      // (doubles of its vectors and tables: for the MPCQP_VERBOSE line)
  int batch = 0, at_map = 0;    // load and write-out phases in batched stages; A' written out from the staged copy of A through Selection::at_map
  int t_parts = 0, sing_k = 0;  // the factorisation's operands on chip: parts of the T tiles in LDS (0: through the slab), entries per column of the singleton list (0: the full pass)
};

// Everything the policy decides for one handle.
struct Selection {
  int err = 0; std::string error;      // SEL_ERR_ARG / SEL_ERR_LIMIT: nothing else is valid then
  int waves = 0;                // 0 = streaming (1 wave / QP), NW > 0 = LDS-resident factor with NW waves / QP
  bool wide = false;            // resident kernel instance that may use the whole register file (one QP per CU)
  bool gblocks = false;         // multi-wave LDL' kernel with the factor blocks streamed from the HBM slab
  bool zyg = false;             // ... with z, y in the slab instead of LDS (lifts workgroups per CU for long horizons)
  bool occ3 = false;            // ... its 168-VGPR instance (exactly 3 workgroups per CU fit in LDS), 8 blocks in flight
  bool occ4 = false;            // ... its 128-VGPR instance (>= 3 workgroups per CU fit in LDS)
  bool res1x = false;           // one-wave kernel, 128-VGPR instance: more than eight QPs per CU when the LDS footprint allows (double integrator N=10: 12.1 -> 13.8 M QP/s)
  int res3 = 0;                 // LDS-resident 4-wave kernel: 3 or 4 workgroups per CU (168- / 128-VGPR instances) when the LDS footprint allows, else 0
  bool stream_pd8 = false;      // streaming kernel instance: 8 blocks in flight when one QP per SIMD is all that fits
  bool oc = false;              // on-chip mode of the global-block kernel (kernel_onchip.hpp): two workgroups per CU, factor in LDS + registers
  int oc8 = 0;                  // ... its eight-wave instances for long chains (one workgroup per CU): 1 = <NG 4, NH 4>, 2 = <NG 7, NH 7>
  bool split = false;           // ... as two kernels, set-up and iteration (kernel_oc_split.hpp): the default; MPCQP_OC_MONO=1 and the tile experiment keep the single kernel
  bool tiles = false;           // on-chip kernels: dense tiles of A for the two sweeps of the iteration (plan.hpp build_tile_plan)
  bool vtiles = false;          // ... in the two-kernel form, on the vector ALUs (kernel_oc_split.hpp; MPCQP_VTILES=1); mpcqp.hip clears it where the table has no such instance
  int resume_rounds = 1;        // two-kernel form: {re-factorisation, iteration} pairs queued behind a solve before the last pair (MPCQP_RESUME_ROUNDS)
  Plan plan; ResPlan rplan; OcPlan ocplan; TilePlan tplan; WsLayout wl;
  std::vector<unsigned short> at_map;  // two-kernel form, A staged: ELL entry of A per ELL entry of A' (plan.hpp build_at_map; empty where it does not apply)
  TLdsPlan tlds; SingList sing; // two-kernel form: what the set-up kernel's factorisation reads on chip (plan.hpp; empty where a knob or the fit says no)
  long lds = 0;                 // dynamic LDS of the iteration (or only) kernel
  long stage = 0;               // on-chip mode: staging doubles of the iteration kernel (plan.hpp oc_stage_doubles) ...
  int a_lds = 0, p_lds = 0;     // ... and whether A's / A's and P's values fit them
  int at_poll = -1, at_free = -1;      // single-kernel four-wave form, MPCQP_LATE: plan.hpp oc_late_chunks
  SetupShape setup;
  std::vector<int> a_assign;    // eight-wave two-kernel form: A's row chunks per wave, 8 x 32 (empty: round-robin); not used with vtiles

  // what mpcqp_plan_info reports in slot 15
  int family() const { return oc ? 200 + waves : gblocks ? 100 + waves : waves; }
  // template arguments of the on-chip instance: the one place that knows a plan without an arrow head runs the instances without hub blocks
  int oc_ng() const { return oc8 > 0 ? OC8_INST[oc8 - 1].ng : OC_NG; }
  int oc_nh() const { return !ocplan.has_hub ? 0 : oc8 > 0 ? OC8_INST[oc8 - 1].nh : OC_NH; }
};

namespace sel {

// what the steps of the rule share
struct Ctx {
  int n, m, batch; const int *Pp, *Pi, *Ap, *Ai; long cus; const Knobs &k;
  bool forced; std::string family;      // a family was asked for (MPCQP_VARIANT or mpcqp_create_tuned), and its name
  bool twist, small_ok;
  int want = -1;                        // waves per QP (0 = streaming), -1 = not decided
  Plan p0, p1, p4;                      // the one-wave plan as it stands, with ELL widths padded, and the multi-wave candidate (becomes the chosen one)
  Plan plan(int ordering, int pad4, int max_sep = 3) const { return build_plan(n, m, Pp, Pi, Ap, Ai, ordering, pad4, max_sep); }
  bool asked(const char *f) const { return forced && family == f; }
};

inline void fail(Selection &s, int code, const std::string &msg) { s.err = code; s.error = msg; }

// does the four-wave on-chip mode take the pattern at two workgroups per CU (in the twisted or the padded-twist order)?
inline bool oc_takes(const Ctx &c) {
  if (c.k.no_oc || !c.small_ok) return false;
  auto ok4 = [&](const Plan &q) { const OcPlan o = build_oc_plan(q, 4, 1 << 20, OC_NG, OC_NH); return o.ok && lds_bytes_oc(q, build_res_plan(q, 4, false), o) <= OC_LDS_MAX; };
  if (ok4(c.p4)) return true;
  // (the padded twist -- plan.hpp ordering 3 -- where the hub variables would otherwise share a block with the last frame and spill into a second one: cart-pole N=22, 25)
  if (!c.twist) return false;
  const Plan q = c.plan(3, 1);
  return q.error.empty() && ok4(q);
}

// MPCQP_VARIANT / mpcqp_create_tuned: the family by name
inline void forced_family(Ctx &c, Selection &s) {
  const std::string &v = c.family;
  if (v == "stream") c.want = 0; else if (v == "res1") c.want = 1; else if (v == "res4") c.want = 4; else if (v == "res8") c.want = 8;
  else if (v == "gres4") { c.want = 4; s.gblocks = true; }
  else if (v == "res2") c.want = 2;
  else if (v == "gres2") { c.want = 2; s.gblocks = true; }
  else if (v == "oc4") { c.want = 4; s.gblocks = true; s.oc = true; }
  else if (v == "oc8") { c.want = 8; s.gblocks = true; s.oc = true; s.oc8 = -1; }
}

// The family by rule.
// measured on MI355X: one wave per QP with the factor in LDS when it is tiny; four waves per QP
// with the factor in LDS when at least two QPs fit per CU; otherwise occupancy beats residency and the factor
// blocks are streamed from the HBM slab by the same LDL' / segment machinery (several workgroups per CU)
inline void family_rule(Ctx &c, Selection &s) {
  const Plan &p1 = c.p1, &p4 = c.p4; const bool small_ok = c.small_ok; int &want = c.want;
  ResPlan r1 = build_res_plan(p1, 1), r4 = build_res_plan(p4, 4);
  const long l1 = lds_bytes_res(p1, r1), l4 = lds_bytes_res(p4, r4);
  // latency regime (measured, tools/graph_tick.py): when the whole batch is resident in one round of 4-wave workgroups
  // (two per CU by registers, one when the factor needs more than half the LDS), four waves per QP with the factor in
  // LDS finish a QP soonest (double integrator x256: 1.12 ms vs 1.41 ms with one wave per QP; quadrotor N=20 x256:
  // 1.21 ms vs 1.96 ms with the factor streamed from HBM)
  const long cus = c.cus;
  // (workgroups of the LDS-resident 4-wave kernel per CU: by LDS, and by the register budget of its instances -- 128 / 168 / 256 VGPRs)
  const long cap4 = (small_ok && l4 <= LDS_MAX) ? std::min<long>(LDS_MAX / l4, l4 <= 40 * 1024 ? 4 : l4 <= 53 * 1024 ? 3 : 2) : 0;
  // two waves per QP (168-VGPR instance: up to six per CU): the two half chains of the twisted order each get a wave and nothing idles in
  // the chain phases.  Taken where it fits more QPs per CU than the 4-wave kernel and at most one fewer than one wave per QP would:
  // double integrator N=20 (28 KiB, five per CU) 1.87 M QP/s against 1.55 M with one wave and 1.46 M with four; at 21-23 KiB +4...8 %
  // over one wave; below 15 KiB one wave per QP (11-13 per CU) wins, at 34 KiB and above the 4-wave kernel; same latency as the 4-wave
  // kernel on a batch of 64-1024
  const ResPlan r2 = build_res_plan(p4, 2);
  const long l2 = lds_bytes_res(p4, r2);
  const long q1 = small_ok && l1 <= LDS_MAX ? LDS_MAX / l1 : 0, q2 = small_ok && l2 <= 40 * 1024 ? std::min<long>(LDS_MAX / l2, 6) : 0;
  if (q2 > cap4 && q2 + 1 >= q1 && !c.k.no_res2) want = 2;
  // the latency regime above; with three or four 4-wave workgroups per CU they stay ahead of one wave per QP up to about three resident
  // rounds (double integrator x2048 1.57 vs 1.81 ms, x4096 2.89 vs 2.76 ms)
  else if (cap4 > 0 && (long)c.batch <= cus * cap4 * (cap4 >= 3 ? 3 : 1)) {
    want = 4;
    // ... and in it the on-chip mode where it takes the pattern: up to two rounds of its two workgroups per CU it finishes a batch sooner than
    // the LDS-resident kernel at any occupancy (tools/small_batch_scan.py, x 64 ... 1024: quadrotor N = 5 / 10 / 20 0.21 / 0.43 / 0.85 ms against
    // 0.24 / 0.52 / 1.08, cart-pole N = 20 / 30 0.73 / 1.12 against 0.89 / 1.41, double integrator N = 30 / 50 1.11 / 1.64 against 1.31 / 2.18)
    if ((long)c.batch <= cus * 4 && oc_takes(c)) { s.gblocks = true; s.oc = true; }
  }
  // one wave per QP only where it puts more QPs on a CU than the 4-wave kernel has workgroups there (five against four at 28 KiB: +6 %;
  // four against four at 34-36 KiB: the 4-wave kernel is 23-31 % ahead -- double integrator N=24 / 26, cart-pole N=15)
  else if (small_ok && l1 <= 40 * 1024 && LDS_MAX / l1 > cap4) want = 1;
  else {
    // The on-chip mode (factor in LDS + registers at two workgroups per CU, solves and factorisation on the matrix cores) wherever the pattern is
    // a block chain with an arrow head that fits it AND the alternative is the LDS-resident 4-wave kernel at two workgroups per CU or a factor
    // streamed from the slab (measured, profiles/r02_final_variant_grid.txt, x 8192: quadrotor N = 6 ... 20 +8 ... +48 %, cart-pole N = 30 / 40 / 50
    // +20 / +26 / +37 %, double integrator N = 40 ... 80 +12 ... +64 %).  With three or more resident workgroups per CU the LDS-resident
    // kernels stay ahead (quadrotor N = 5 2.57 vs 2.06 M QP/s, cart-pole N = 20 818k vs 656k, double integrator N = 30 792k vs 611k).
    // LDS-resident 4-wave kernel while two fit a CU
    if (small_ok && l4 <= 80 * 1024) { want = 4; if (l4 > 53 * 1024 && oc_takes(c)) { s.gblocks = true; s.oc = true; } }
    // factor streamed from the slab, two waves per QP (168-VGPR instance, six workgroups per CU) while six fit the LDS: ahead of four waves x
    // four workgroups there (double integrator N=100 145k -> 156k QP/s; at 32 KiB and above four waves win)
    else if (small_ok && !c.k.no_res2 && lds_bytes_res_gb(p4, build_res_plan(p4, 2, true)) <= LDS_MAX / 6) {
      want = 2; s.gblocks = true;
      if (oc_takes(c)) { want = 4; s.oc = true; }
    }
    else if (small_ok && lds_bytes_res_gb(p4, build_res_plan(p4, 4, true), !c.k.no_zyg) <= LDS_MAX) { want = 4; s.gblocks = true; s.oc = oc_takes(c); }
    else want = 0;
  }
}

// Long chains: where the rule arrives at a factor streamed from the slab, the eight-wave on-chip instances take the pattern if it is
// a block chain with an arrow head of up to 56 blocks that fits one CU (MPCQP_NO_OC8 keeps the global-block kernels)
inline void eight_wave_takeover(Ctx &c, Selection &s) {
  if (!((s.oc8 < 0 || (c.want > 0 && s.gblocks && !s.oc && !c.forced && !c.k.no_oc8 && !c.k.no_oc)) && c.small_ok)) return;
  auto take = [&](const Plan &p, const OcPlan &o, int k) { s.ocplan = o; s.oc8 = k + 1; s.oc = true; s.gblocks = true; s.zyg = OC8_INST[k].zyg; c.want = 8; c.p4 = p; };
  Plan p8 = c.plan(c.twist ? 3 : -1, 2);
  s.oc8 = 0;
  if (c.twist && !c.k.no_dissect) {
    // the dissected order first (plan.hpp build_plan ordering 4): separators of the stage chain in the hub block where it has room, several twisted pairs of
    // short chains instead of one pair of long ones
    Plan pd = c.plan(4, 2);
    if (pd.error.empty()) {
      const ResPlan rd = build_res_plan(pd, 8, false);
      for (int k = 0; k < 2 && !s.oc8; k++) {
        const OcPlan o = build_oc_plan(pd, 8, 1 << 20, OC8_INST[k].ng, OC8_INST[k].nh, OC8_MAX_CHAIN);
        if (o.ok && o.has_hub && o.pairs.size() > 1 && lds_bytes_oc(pd, rd, o, OC8_INST[k].zyg) <= OC8_LDS_MAX) take(pd, o, k);
      }
    }
  }
  if (!s.oc8 && p8.error.empty()) {
    const ResPlan r8 = build_res_plan(p8, 8, false);
    for (int k = 0; k < 2 && !s.oc8; k++) {
      const OcPlan o = build_oc_plan(p8, 8, 1 << 20, OC8_INST[k].ng, OC8_INST[k].nh, OC8_MAX_CHAIN);
      // (a pattern without an arrow head -- the reduced form -- runs the same instances with no hub block: two-kernel form only)
      if (o.ok && (o.has_hub || !c.k.oc_mono) && lds_bytes_oc(p8, r8, o, OC8_INST[k].zyg) <= OC8_LDS_MAX) take(p8, o, k);
    }
  }
  if (!s.oc8 && c.asked("oc8")) fail(s, SEL_ERR_LIMIT, "the eight-wave on-chip variant does not take this pattern / size");
}

// Four-wave on-chip mode: block tridiagonal + arrow patterns whose factor fits LDS + the registers of the instance at two workgroups per CU;
// which order of the chain (twisted, padded twist, dissected with one separator), or not at all
inline void four_wave_order(Ctx &c, Selection &s) {
  if (!(s.oc && !s.oc8)) return;
  Plan &p4 = c.p4; const bool small_ok = c.small_ok, twist = c.twist;
  const ResPlan r4 = build_res_plan(p4, 4, false);
  s.oc = false;
  OcPlan o = small_ok ? build_oc_plan(p4, 4, 1 << 20, OC_NG, OC_NH) : OcPlan();
  bool dissected4 = false, padded4 = false;
  if (small_ok && twist && !c.k.no_padtwist) {
    // the padded twist (ordering 3: the hub moved up to a block boundary, the chain part whole blocks) where the plain order is not taken -- the hub shares a
    // block with the last frame and spills into a second one: cart-pole N=22, 25 fell to the LDS-resident kernel, 18 ms against 12 -- or leaves one long chain
    // where the twist has two (cart-pole N=24: one chain of 7)
    Plan q = c.plan(3, 2);
    if (q.error.empty()) {
      const OcPlan oq = build_oc_plan(q, 4, 1 << 20, OC_NG, OC_NH);
      auto longest = [](const OcPlan &x) { return std::max(x.chainE.size(), x.chainF.size()); };
      const bool fits = oq.ok && lds_bytes_oc(q, build_res_plan(q, 4, false), oq) <= OC_LDS_MAX, o_fits = o.ok && lds_bytes_oc(p4, r4, o) <= OC_LDS_MAX;
      if (fits && (!o_fits || longest(oq) < longest(o))) { o = oq; p4 = q; padded4 = true; }
    }
  }
  if (o.ok && o.has_hub && twist && !c.k.no_dissect && !c.k.oc_mono && !c.k.tiles && !c.k.vtiles && c.k.doubles < 0) {
    // the dissected order with one separator: two twisted pairs on the four waves (plan.hpp build_plan ordering 4; its own kernel instances, two-kernel form only)
    Plan pd = c.plan(4, 2, 1);
    if (pd.error.empty()) {
      const OcPlan od = build_oc_plan(pd, 4, 1 << 20, OC_NG, OC_NH);
      if (od.ok && od.pairs.size() == 2 && lds_bytes_oc(pd, build_res_plan(pd, 4, false), od) <= OC_LDS_MAX) { o = od; p4 = pd; dissected4 = true; }
    }
  }
  if (o.ok && (dissected4 || padded4 || lds_bytes_oc(p4, r4, o) <= OC_LDS_MAX)) {
    s.ocplan = o; s.oc = true;
    // same ordering and blocks, ELL widths for this instance's 8 slots in flight (plan.hpp build_ell pad = 2)
    if (!dissected4 && !padded4 && !c.k.oc_pad4) { Plan poc = c.plan(twist ? 2 : -1, 2); if (poc.error.empty() && poc.nblk == p4.nblk) p4 = poc; }
  }
  if (!s.oc && c.want == 4 && c.asked("oc4")) fail(s, SEL_ERR_LIMIT, "the on-chip variant does not take this pattern / size");
}

// EXPERIMENTAL, opt-in (MPCQP_TILES=1): dense tiles for the two sweeps of the iteration where the pattern has them (dense Jacobian
// blocks: the quadrotor's 12 x 16 per stage) and the LDS still fits.  Parity-green, but measured SLOWER than the ELL sweeps in these
// register-bound instances (quadrotor N = 20 x 8192: 12.0 - 13.7 ms against 8.68), so the default stays ELL.
inline void experiment_tiles(const Ctx &c, Selection &s) {
  if (!(s.oc && s.ocplan.has_hub && c.k.tiles == 2)) return;
  const Plan &pl = s.plan;
  s.tplan = build_tile_plan(pl, c.n, c.m, c.Ap, c.Ai, 2);
  s.tiles = s.tplan.on && s.tplan.max_per_block <= 1 && s.tplan.max_per_chunk <= 8 && s.tplan.rows_consecutive &&
            pl.A.nchunks <= 3 * c.want && pl.At.nchunks <= 2 * c.want &&      // (kernel_onchip.hpp OC_TILE_MAXA / OC_TILE_MAXT chunk records per wave)
            lds_bytes_oc(pl, s.rplan, s.ocplan, s.oc8 && s.zyg, &s.tplan) <= (s.oc8 ? OC8_LDS_MAX : OC_LDS_MAX);
  if (s.tiles) s.wl = ws_layout(pl, &s.tplan);
}

// EXPERIMENT, opt-in (MPCQP_VTILES=1): the two sweeps of the iteration on ONE copy of A's dense blocks -- 16 x 16 tiles, row-major in the slab, multiplied
// on the vector ALUs (kernel_oc_split.hpp) -- plus the remainder ELL layouts.  No LDS beyond the ELL form's.  The set-up still writes the two ELL copies:
// the residual sweeps of the termination checks and the factorisation read them.
inline void experiment_vtiles(const Ctx &c, Selection &s) {
  if (!(s.oc && !s.tiles && c.k.vtiles == 2 && !c.k.oc_mono)) return;
  const Plan &pl = s.plan;
  s.tplan = build_tile_plan(pl, c.n, c.m, c.Ap, c.Ai, 2);
  bool fits = s.tplan.on && s.tplan.max_per_block <= 1 && s.tplan.max_per_chunk <= 8 && s.tplan.rows_consecutive &&
              pl.A.nchunks <= 8 * c.want && pl.At.nchunks <= 16 * c.want;          // (a wave's tile records ride in the lanes of registers: 8 tiles x 8 chunks of A, 4 blocks x 16 chunks of A')
  for (int t = 0; t < s.tplan.ntile && fits; t++) {
    int first = -1; for (int r = 0; r < BS; r++) if (s.tplan.rowid[(size_t)t * BS + r] >= 0) { first = s.tplan.rowid[(size_t)t * BS + r]; break; }
    fits = first >= 0 && first + BS <= pl.mpad;                                 // (a tile's sixteen rows of w are read as they lie: all inside the vector)
  }
  s.vtiles = fits;
  if (s.vtiles) s.wl = ws_layout(pl, &s.tplan);
}

// EXPERIMENT, opt-in (MPCQP_DOUBLES=<n>): double stages of the solve (plan.hpp oc_add_doubles) where the CU's LDS has room for their product blocks
// beside the factor: every one takes a dependent 16 x 16 mat-vec off the critical path of both triangular sweeps.  Parity-green, but measured
// SLOWER (cart-pole N=100: 29.1 against 27.8 ms): the four wave-parallel phases it adds (two mat-vecs per double stage and direction, 48 cycles
// of matrix pipe per MFMA, four more barriers) cost more than the halved chains save.
inline void experiment_doubles(const Ctx &c, Selection &s, long &need) {
  if (!(s.oc && !s.tiles && c.k.doubles >= 0)) return;
  const long cap = s.oc8 ? OC8_LDS_MAX : OC_LDS_MAX;
  int nd = (int)std::max<long>(0, (cap - need) / (BLK * 8));
  nd = std::min(nd, c.k.doubles);
  for (; nd > 0; nd--) {       // (the table grows with the stages: take as many as still fit)
    OcPlan o2 = s.ocplan; oc_add_doubles(o2, nd);
    const long n2 = lds_bytes_oc(s.plan, s.rplan, o2, s.oc8 && s.zyg, nullptr);
    if (n2 <= cap) { s.ocplan = o2; need = n2; break; }
  }
}

// register / occupancy instances of the family that was chosen, from its LDS footprint
inline void occupancy_instances(const Ctx &c, Selection &s, long &need) {
  const Plan &pl = s.plan; const int want = c.want;
  if (s.gblocks && !s.oc && want == 4 && !c.k.no_zyg) {     // (the two-wave global-block kernel has no such instance: forced on a long horizon it took this layout and returned garbage)
    // long horizons: with z and y in the slab one more workgroup fits per CU (2 -> 3 or 1 -> 2); measured on quadrotor N=50
    const long alt = lds_bytes_res_gb(pl, s.rplan, true);
    const long fit = LDS_MAX / need, fit_alt = std::min<long>(LDS_MAX / alt, 3);
    if (fit <= 2 && fit_alt > fit) { s.zyg = true; need = alt; }
  }
  s.occ4 = s.gblocks && !s.oc && !s.zyg && need <= 53 * 1024 && !c.k.gb_occ2;
  // LDS between 40 and 53 KiB: three workgroups per CU fit, so the instance compiled for three waves per SIMD (168 VGPRs, no
  // spills, 8 blocks in flight) replaces the 128-VGPR one (at 42 KiB 92.9k -> 95.8k QP/s on cart-pole N=100, which now fits four per CU
  // because the temp tiles alias w, plan.hpp gb_tmp_alias: 76.2 -> 73.2 ms per 8192; at 32 KiB it loses, 589k -> 551k)
  // (with z and y in the slab the 168-VGPR instance at three per CU also beats the 128-VGPR one at four: quadrotor N=50 23.9 vs 26.0 ms)
  s.occ3 = s.gblocks && !s.oc && need <= 53 * 1024 && (need > 40 * 1024 || s.zyg || c.k.gb_occ3) && !c.k.gb_occ2;
  if (!c.small_ok || need > LDS_MAX) return fail(s, SEL_ERR_LIMIT, "resident variant needs " + std::to_string(need) + " B of LDS");
  // (kernel_onchip.hpp oc_load_factor keeps a wave's share of the fill list in the lanes of one register: 21 records of three)
  if (s.oc && s.ocplan.nfill > 21 * want) return fail(s, SEL_ERR_LIMIT, "on-chip variant: " + std::to_string(s.ocplan.nfill) + " factor blocks to load exceed 21 per wave");
  s.lds = need;
  s.res1x = want == 1 && !s.gblocks && LDS_MAX / need > 8 && !c.k.no_res1x;
  if (!s.gblocks && want == 4 && !c.k.no_res3) s.res3 = need <= 40 * 1024 ? 4 : need <= 53 * 1024 ? 3 : 0;
  s.lds = std::max<long>(s.lds, c.k.lds_min);   // experiment: limit workgroups per CU
}

// On-chip mode: one kernel or two, what the iteration kernel stages, and the set-up kernel's own launch shape.
inline void oc_launch_shape(const Ctx &c, Selection &s) {
  const Plan &pq = s.plan; const OcPlan &o = s.ocplan; const int nw = s.waves;
  s.stage = oc_stage_doubles(o, s.rplan, pq);
  // (single-kernel four-wave instance only: the eight-wave solve, oc_solve_long, has no ticket wait, and the two-kernel form sweeps all of A' up front)
  s.split = !s.tiles && !c.k.oc_mono && pq.A.nchunks <= 32 * nw && pq.At.nchunks <= 32 * nw;      // (a wave's chunk offsets ride in the lanes of one register: kernel_oc_split.hpp oc_my_chunks)
  if (!s.split) s.vtiles = false;
  s.resume_rounds = c.k.resume_rounds;
  // (opt-in since the chains run on the 4-block MFMA: they now reach the ticket before wave 3 has the rows -- 913k with, 917k without)
  if (c.k.late && !s.tiles && !s.oc8 && !s.split) oc_late_chunks(pq, o, 4, 3 /* OC_POLL_TRIP */, &s.at_poll, &s.at_free);
  s.a_lds = (long)pq.A.entries() <= s.stage ? 1 : 0;
  s.p_lds = s.a_lds && (long)pq.A.entries() + (long)pq.P.entries() <= s.stage ? 1 : 0;
  SetupShape &su = s.setup;
  su.nw = nw; su.lds = s.lds; su.stage = s.stage; su.a_lds = s.a_lds; su.p_lds = s.p_lds;
  if (!s.split) return;
  // The set-up as four-wave workgroups with their own LDS request -- the factorisation's scratch blocks and assembly records, the staged values of A
  // and P where they fit, their 16-bit index tables where those fit too -- and their own vector layout: q stays in the slab, z is never touched, y
  // holds one n-vector of the Ruiz passes (kernel_oc_split.hpp oc_lds).  Three workgroups per CU (the kernel's 164 VGPRs allow no more) beat two
  // wherever A's values still fit beside them, and so does an unstaged third against a half-staged pair; a fully staged pair beats an unstaged
  // three.  Measured (x 8192 unless said, set-up kernel, ms): quadrotor N=20 A + P + index tables at two per CU 2.47, A alone at three 2.35, nothing
  // staged at three 3.26 (round-4 mid build); cart-pole N=50 2.14 / 1.95; cart-pole N=100 A staged at two 4.28, nothing staged at three 3.99;
  // quadrotor N=50 nothing fits: two per CU 8.05, squeezed to three 8.55 (not taken: the footprint is what the layout needs).  DESIGN.md 3.9
  const long scratch = 8L * BLK + ((4L * pq.nblk + 15) / 16) * 16;                 // (plan.hpp oc_stage_doubles: OC_LDL_SCR blocks + the assembly records)
  const long vec = 2L * pq.npad + oc_rext(nw, std::max<int>(1, (int)o.pairs.size())) + pq.mpad + pq.npad + 16L * 4 + 16 + 16L * 4;      // x, r; w; y (an n-vector here); the reduction scratch
  const long tabw = ((long)o.o_pos + 1) / 2 + 4 + ((long)pq.A.nchunks + pq.At.nchunks + pq.P.nchunks + 3 + 1 + 1) / 2;
  const long cu = LDS_MAX, nA = (long)pq.A.entries(), nP = (long)pq.P.entries();
  struct Shape { long stage, bytes; int a, p, ix16, zpad, ixo_a, ixo_p; bool fits; };
  const long zoff = 2L * pq.npad + oc_rext(nw, std::max<int>(1, (int)o.pairs.size()));      // (the z region starts behind x and r: kernel_oc_split.hpp oc_lds<NW, true>)
  auto shape = [&](const long cap_bytes) {
    const long cap = cap_bytes / 8;
    Shape r{scratch, 0, 0, 0, 0, 0, 0, 0, false};
    if (std::max(scratch, nA) + vec + tabw <= cap) { r.stage = std::max(scratch, nA); r.a = 1; }
    if (r.a && std::max(scratch, nA + nP) + vec + tabw <= cap) { r.stage = std::max(scratch, nA + nP); r.p = 1; }
    r.stage = (r.stage + 15) / 16 * 16;
    long total = r.stage + vec + tabw;
    const long zA = (nA / 4 + 15) / 16 * 16, zP = (nP / 4 + 15) / 16 * 16, zAP = ((nA + nP) / 4 + 15) / 16 * 16;
    const bool ix_ok = pq.npad < 65536 && !c.k.no_ix16;
    if (r.a && r.p && ix_ok) {      // (the ten Ruiz passes then gather without a round trip to the L2 in front of every batch)
      if (total + zAP <= cap) { r.ix16 = 3; r.zpad = (int)zAP; } else if (total + zA <= cap) { r.ix16 = 1; r.zpad = (int)zA; }
      r.ixo_a = (int)(4 * (r.stage + zoff)); r.ixo_p = r.ixo_a + (int)nA;
      total += r.zpad;
    } else if (!r.a && ix_ok) {
      // values in the slab: the index tables alone (a quarter less to read per pass, the gathers' addresses from LDS) -- one of them in the factorisation's
      // scratch, which is idle until the factorisation starts, the other in the z region where that does not cost a workgroup per CU
      const bool a_scr = zA <= r.stage, p_scr = zP <= r.stage;
      auto z_fits = [&](long z) { return total + z <= cap && cu / ((total + z) * 8) == cu / (total * 8); };
      if (a_scr && z_fits(zP)) { r.ix16 = 3; r.ixo_a = 0; r.zpad = (int)zP; r.ixo_p = (int)(4 * (r.stage + zoff)); }
      else if (p_scr && z_fits(zA)) { r.ix16 = 3; r.ixo_p = 0; r.zpad = (int)zA; r.ixo_a = (int)(4 * (r.stage + zoff)); }
      else if (a_scr) { r.ix16 = 1; r.ixo_a = 0; }
      else if (z_fits(zA)) { r.ix16 = 1; r.zpad = (int)zA; r.ixo_a = (int)(4 * (r.stage + zoff)); }
      total += r.zpad;
    }
    r.bytes = total * 8; r.fits = total <= cap;
    return r;
  };
  Shape sh = shape(cu / 2);
  if (c.k.setup_cap != LONG_MIN) sh = shape(c.k.setup_cap);
  else { const Shape s3 = shape(cu / 3); if (s3.fits && (s3.a || !(sh.a && sh.p))) sh = s3; }
  su.a_lds = sh.a; su.p_lds = sh.p; su.ix16 = sh.ix16; su.zpad = sh.zpad; su.ixo_a = sh.ixo_a; su.ixo_p = sh.ixo_p;
  su.stage = sh.stage; su.nw = 4; su.lds = sh.bytes; su.vecs = vec + sh.zpad; su.tabw = tabw;
  // the factorisation's operands on chip: fitted to the LDS this shape already asks for, never a reason to ask for more
  if (!c.k.no_t_lds) s.tlds = build_t_lds_plan(pq, su.stage);
  if (!c.k.no_sing_list) s.sing = build_sing_list(pq);
  su.t_parts = s.tlds.parts; su.sing_k = s.sing.K;
  su.batch = (c.k.no_setup_batch || pq.m <= 0 || pq.A.entries() <= 0 || pq.P.entries() <= 0) ? 0 : 1;      // (its masked loads clamp their addresses into the arrays: none may be empty)
  if (su.batch && su.a_lds) s.at_map = build_at_map(pq);
  su.at_map = s.at_map.empty() ? 0 : 1;
  if (s.oc8 && !c.k.no_abalance) {
    // row chunks of A to waves by longest-processing-time over their load batches (a batch = one round trip to memory; plan.hpp ell_batches8)
    std::vector<int> assign(8 * 32, -1), load(8, 0), cnt(8, 0), order_(pq.A.nchunks);
    for (int ch = 0; ch < pq.A.nchunks; ch++) order_[ch] = ch;
    auto batches = [&](int ch) { return ell_batches8(pq.A.chunk_off[ch + 1] - pq.A.chunk_off[ch]); };
    std::stable_sort(order_.begin(), order_.end(), [&](int a, int b) { return batches(a) > batches(b); });
    bool okA = true;
    for (int ch : order_) {
      int w = 0;
      for (int v = 1; v < 8; v++) if (load[v] < load[w] || (load[v] == load[w] && cnt[v] < cnt[w])) w = v;
      if (cnt[w] >= 32) { okA = false; break; }
      assign[w * 32 + cnt[w]++] = ch; load[w] += std::max(1, batches(ch));
    }
    if (okA) s.a_assign = assign;
  }
}

}  // namespace sel

// Which compiled kernel instance a Selection launches: the one mapping from the policy's flags to the template arguments of the k_*.hip units
// (kernel_table.hpp).  Host-only; mpcqp.hip turns a KernelId into a table pointer and does nothing else with the flags, and the tests read the
// same mapping through tests/support/plan_interp.cpp (tests/support/instance_cases.py: the census of the instances and who reaches them).
enum KernelKind { K_STREAM = 0, K_LDS, K_GB, K_OC_MONO, K_OC_SETUP, K_OC_ADMM, K_OC_ADMM_RF, K_OC_ADMM_P4, K_OC_ADMM_TL, K_OC_RESCALE };
struct KernelId {
  int kind = K_STREAM;
  int nw = 0, minw = 0;       // waves per QP; K_LDS / K_GB: the register budget as waves per SIMD (4 = 128, 3 = 168, 2 = 256 VGPRs; 1 = the whole file)
  int zyg = 0;                // K_GB: z, y in the slab
  int ng = 0, nh = 0;         // on-chip instances: positions and hub blocks per wave in registers (nh = 0: the instance without hub blocks)
  int hub = 0;                // K_OC_SETUP / K_OC_RESCALE: the instance for patterns with an arrow head
  int pd = 0;                 // K_STREAM: factor blocks in flight (4 or 8)
  int reuse = 0;              // the kept-workspace twin (_r1 units; K_OC_SETUP: its reuse instance)
  int rf = 0;                 // K_OC_ADMM_P4: the instance that re-factorises in place (K_OC_ADMM_RF is a kind of its own)
  int tiles = 0;              // K_OC_MONO: the tile experiment's instance
  int soft = 0;               // K_OC_ADMM / K_OC_ADMM_RF / K_OC_ADMM_P4: the soft-row twin (mpcqp_set_soft_rows; k_oc_admm_soft*.hip)
};
// the streaming kernel of a handle without resident waves
inline KernelId stream_kernel_id_of(const Selection &s) { KernelId k; k.kind = K_STREAM; k.nw = 1; k.pd = s.stream_pd8 ? 8 : 4; return k; }
// the single kernel of a resident handle: waves per QP, register budget, factor location, and the kept-workspace twin.  (On-chip: the single-kernel form's
// lookup, which a two-kernel handle never launches; a plan without an arrow head asks with nh = 0, for which the eight-wave table has no instance.)
inline KernelId res_kernel_id_of(const Selection &s, bool reuse) {
  KernelId k; k.reuse = reuse ? 1 : 0;
  auto lds = [&](int nw, int minw) { k.kind = K_LDS; k.nw = nw; k.minw = minw; return k; };
  auto gb = [&](int nw, int minw, bool zyg) { k.kind = K_GB; k.nw = nw; k.minw = minw; k.zyg = zyg ? 1 : 0; return k; };
  if (s.oc) { k.kind = K_OC_MONO; k.nw = s.oc8 ? 8 : 4; k.minw = 2; k.ng = s.oc_ng(); k.nh = s.oc_nh(); k.hub = s.ocplan.has_hub ? 1 : 0; k.tiles = s.tiles ? 1 : 0; return k; }
  if (s.gblocks && s.waves == 2) return gb(2, 3, false);
  if (s.gblocks && s.zyg) return gb(4, s.occ3 ? 3 : 2, true);
  if (s.gblocks && s.occ3) return gb(4, 3, false);
  if (s.gblocks) return gb(4, s.occ4 ? 4 : 2, false);
  if (s.waves == 1) return lds(1, s.res1x ? 4 : 2);
  if (s.waves == 8) return lds(8, 2);
  if (s.waves == 2) return lds(2, 3);
  if (s.res3 == 4) return lds(4, 4);
  if (s.res3 == 3) return lds(4, 3);
  return lds(4, s.wide ? 1 : 2);
}
// the kernels of the two-kernel on-chip form: the set-up (in its own launch shape), the kernel that takes its place after mpcqp_update_matrices, the iteration
inline KernelId oc_setup_kernel_id_of(const Selection &s, bool reuse) { KernelId k; k.kind = K_OC_SETUP; k.nw = s.setup.nw; k.hub = s.ocplan.has_hub ? 1 : 0; k.reuse = reuse ? 1 : 0; return k; }
inline KernelId oc_rescale_kernel_id_of(const Selection &s) { KernelId k; k.kind = K_OC_RESCALE; k.nw = s.setup.nw; k.hub = s.ocplan.has_hub ? 1 : 0; return k; }
// soft: the handle has soft rows set -- the twin of the same shape; the tile experiment has none (mpcqp_set_soft_rows refuses such a handle)
inline KernelId oc_admm_kernel_id_of(const Selection &s, bool rf, bool soft = false) {
  KernelId k; k.nw = s.oc8 ? 8 : 4; k.ng = s.oc_ng(); k.nh = s.oc_nh(); k.hub = s.ocplan.has_hub ? 1 : 0;
  if (!s.oc8 && s.ocplan.pairs.size() > 1) { k.kind = K_OC_ADMM_P4; k.rf = rf ? 1 : 0; k.soft = soft ? 1 : 0; return k; }      // (four waves, two twisted pairs: its own instances)
  if (s.vtiles && !rf) { k.kind = K_OC_ADMM_TL; return k; }      // (the last launch of a solve, rf, runs the ELL sweeps: the set-up writes both forms)
  k.kind = rf ? K_OC_ADMM_RF : K_OC_ADMM; k.soft = soft ? 1 : 0;
  return k;
}
// the iteration (or only) kernel of a handle; rf: the last launch of a two-kernel solve, which re-factorises in place; soft: with soft rows set (two-kernel form
// only: every other family's id keeps soft = 0, and mpcqp_set_soft_rows answers MPCQP_ERR_LIMIT there)
inline KernelId kernel_id_of(const Selection &s, bool reuse, bool rf, bool soft = false) {
  return s.waves == 0 ? stream_kernel_id_of(s) : s.split ? oc_admm_kernel_id_of(s, rf, soft) : res_kernel_id_of(s, reuse);
}
// which handles take soft rows: the two-kernel on-chip form without the tile experiment
inline bool takes_soft_rows(const Selection &s) { return s.waves > 0 && s.oc && s.split && !s.tiles && !s.vtiles; }

// DevOc.su_path of a two-kernel handle's set-up kernel (kernel_onchip.hpp): which of its on-chip and batched paths this handle takes
inline int setup_path_bits(const Selection &s) {
  const SetupShape &u = s.setup;
  return !s.split ? 0 : (u.t_parts > 0 ? 1 : 0) | (u.sing_k > 0 ? 2 : 0) | (u.batch ? 4 : 0) | (u.at_map ? 8 : 0);
}
// The MPCQP_VERBOSE line of a two-kernel handle, up to what only the device knows (mpcqp.hip adds the resident workgroups)
inline std::string setup_shape_text(const Selection &s) {
  const SetupShape &u = s.setup;
  char buf[512];
  snprintf(buf, sizeof(buf), "mpcqp: set-up kernel shape: 4 waves, %ld B of LDS (values of A %s, of P %s, 16-bit index tables %s; A %ld + P %ld entries, vectors %ld, tables %ld doubles), iteration kernel %ld B",
           u.lds, u.a_lds ? "staged" : "in the slab", u.p_lds ? "staged" : "in the slab", u.ix16 == 3 ? "A and P" : u.ix16 ? "A" : "off", (long)s.plan.A.entries(), (long)s.plan.P.entries(), u.vecs, u.tabw, s.lds);
  return buf;
}

// the 16 numbers of mpcqp_plan_info and the 12 of mpcqp_oc_info (include/mpcqp.h)
inline void plan_info_of(const Selection &s, int n, int m, int batch, long *o) {
  const Plan &pl = s.plan;
  o[0] = n; o[1] = m; o[2] = batch; o[3] = pl.npad; o[4] = pl.mpad; o[5] = pl.nb; o[6] = pl.nblk; o[7] = s.lds;
  o[8] = s.wl.stride * 8; o[9] = pl.ordering; o[10] = pl.nnzP_triu; o[11] = pl.nnzA_in; o[12] = pl.nT; o[13] = s.oc ? ((s.tiles || s.vtiles) ? s.tplan.ntile : 0) : (long)pl.fac.size();
  o[14] = pl.A.slots() + pl.At.slots() + pl.P.slots(); o[15] = s.family();
}
inline void oc_info_of(const Selection &s, long *o) {
  for (int k = 0; k < 12; k++) o[k] = 0;
  o[8] = s.plan.A.slots(); o[9] = s.plan.At.slots(); o[10] = s.plan.P.slots();
  if (!s.oc) return;
  const OcPlan &p = s.ocplan;
  o[0] = p.nbc; o[1] = p.has_hub; o[2] = (long)p.chainE.size(); o[3] = (long)p.chainF.size(); o[4] = p.nlds; o[5] = p.npw; o[6] = p.nhr; o[7] = s.split ? 1 + s.resume_rounds : 0; o[11] = (long)std::max<size_t>(1, p.pairs.size());
}

// Kernel shape, from measured rules (profiles/r01_variant_grid.txt): factor in LDS with one, two or four waves per
// QP while enough QPs fit a CU, else the factor streamed from the HBM slab, or brought on chip.  forced_family: nullptr = MPCQP_VARIANT if set, else
// the rule; "" = the rule whatever the environment says; else the family by name (mpcqp_create_tuned).  cus = compute units of the device.
inline Selection select_kernel(int n, int m, int batch, const int *Pp, const int *Pi, const int *Ap, const int *Ai, long cus, const char *forced_family, const Knobs &knobs) {
  Selection s;
  sel::Ctx c{n, m, batch, Pp, Pi, Ap, Ai, cus > 0 ? cus : 256, knobs};
  c.forced = forced_family ? forced_family[0] != 0 : knobs.variant_named;
  c.family = forced_family ? forced_family : knobs.variant;
  c.p0 = c.plan(-1, 0);
  if (!c.p0.error.empty()) { sel::fail(s, SEL_ERR_ARG, c.p0.error); return s; }
  if (c.forced) sel::forced_family(c, s);
  // candidate plans of the multi-wave kernels: ELL chunk widths padded to multiples of 4 (fewer load batches per chunk)
  // and the stage chain eliminated from both ends (two concurrent half-length chains)
  c.twist = !knobs.no_twist;
  c.p1 = c.plan(-1, 1);
  c.p4 = c.plan(c.twist ? 2 : -1, 1);
  if (!c.p1.error.empty() || c.p1.nblk > c.p0.nblk) c.p1 = c.p0;
  if (!c.p4.error.empty() || c.p4.nblk > c.p0.nblk) c.p4 = c.p1;
  c.small_ok = c.p0.nblk < 4096 && c.p0.nb < 512;
  if (c.want < 0) sel::family_rule(c, s);
  sel::eight_wave_takeover(c, s);
  if (s.err) return s;
  sel::four_wave_order(c, s);
  if (s.err) return s;
  // from here on there is one plan: the chosen one
  s.waves = c.want;
  s.plan = c.want >= 2 ? std::move(c.p4) : c.want == 1 ? std::move(c.p1) : std::move(c.p0);
  s.wl = ws_layout(s.plan);
  s.lds = lds_bytes(s.plan);
  if (c.want > 0) {
    s.rplan = build_res_plan(s.plan, c.want, s.gblocks && !s.oc);
    sel::experiment_tiles(c, s);
    sel::experiment_vtiles(c, s);
    long need = s.oc ? lds_bytes_oc(s.plan, s.rplan, s.ocplan, s.oc8 && s.zyg, s.tiles ? &s.tplan : nullptr) : s.gblocks ? lds_bytes_res_gb(s.plan, s.rplan) : lds_bytes_res(s.plan, s.rplan);
    sel::experiment_doubles(c, s, need);
    sel::occupancy_instances(c, s, need);
    if (s.err) return s;
  }
  if (s.lds > LDS_MAX) { sel::fail(s, SEL_ERR_LIMIT, "LDS footprint " + std::to_string(s.lds) + " B exceeds 160 KiB per CU"); return s; }
  if (s.oc) sel::oc_launch_shape(c, s);
  s.wide = s.waves == 4 && s.lds > 80 * 1024;
  s.stream_pd8 = s.lds > 40 * 1024 && !knobs.pd4;   // streaming kernel: 8 blocks in flight when one QP per SIMD is all that fits
  return s;
}

}  // namespace mpcqp
