// t_lds_interp.cpp -- test infrastructure: what the set-up kernel's factorisation reads on chip (csrc/plan.hpp build_t_lds_plan, build_sing_list,
// oc_setup_tables), for the pattern's handle as the library's own selection makes it (csrc/select.hpp select_kernel with the knobs of the environment).
// Host only.  tests/test_t_lds_plan_host.py checks the tables and re-assembles M from them.
#include <cstring>
#include <string>
#include <vector>
#include "../../optimal_control_problem_amd/csrc/plan.hpp"
#include "../../optimal_control_problem_amd/csrc/select.hpp"

using namespace mpcqp;

extern "C" int t_lds_off_host(int r, int c) { return t_lds_off(r, c); }

// info: {two-kernel form, set-up LDS bytes, set-up stage doubles, SetupShape.t_parts, SetupShape.sing_k, build_t_lds_plan(plan, stage).parts (the fit function,
//        called on its own), cap, rec_off, nblk, nT, npad, mpad, n, m, nb, T_LDS_MAX_PARTS, vector doubles of the set-up's layout, table doubles}
// buf:   the arrays below one after the other, each as {length, values ...}; returns the ints written, or -(error) / -100 when cap is too small
extern "C" long t_lds_describe(int n, int m, int batch, const int *Pp, const int *Pi, const int *Ap, const int *Ai, int cus, const char *forced_family, long *info, int *buf, long cap) {
  const Selection s = select_kernel(n, m, batch, Pp, Pi, Ap, Ai, cus, forced_family, Knobs::from_env());
  if (s.err) return -s.err;
  const Plan &pl = s.plan; const TLdsPlan &tp = s.tlds; const SetupShape &su = s.setup;
  const TLdsPlan fit = s.split ? build_t_lds_plan(pl, su.stage) : TLdsPlan();
  const long v[18] = {s.split, su.lds, su.stage, su.t_parts, su.sing_k, fit.parts, fit.cap, fit.rec_off, pl.nblk, pl.nT, pl.npad, pl.mpad, pl.n, pl.m, pl.nb, T_LDS_MAX_PARTS, su.vecs, su.tabw};
  std::copy(v, v + 18, info);
  std::vector<int> tiles_ptr{0}, tiles;
  for (const auto &t : tp.tiles) { tiles.insert(tiles.end(), t.begin(), t.end()); tiles_ptr.push_back((int)tiles.size()); }
  const std::vector<int> tables = oc_setup_tables(pl, s.tlds, s.sing);
  const std::vector<int> *arr[] = {&tp.blk0, &tp.image, &tp.sc_ptr, &tp.sc, &tp.rec, &tp.ta, &tp.tb, &tiles_ptr, &tiles,
                                   &pl.tpos, &pl.asm_ptr, &pl.asm_a, &pl.asm_b, &pl.blk_diag, &pl.asm_pidx, &pl.blkI, &pl.blkJ, &pl.pos, &pl.perm,
                                   &pl.A.chunk_off, &pl.A.src, &pl.At.chunk_off, &pl.At.src, &pl.At.idx, &pl.At.flag, &pl.P.src,
                                   &s.sing.ent, &s.sing.row, &tables};
  long w = 0;
  for (const std::vector<int> *a : arr) {
    if (w + 1 + (long)a->size() > cap) return -100;
    buf[w++] = (int)a->size();
    std::copy(a->begin(), a->end(), buf + w); w += (long)a->size();
  }
  return w;
}
