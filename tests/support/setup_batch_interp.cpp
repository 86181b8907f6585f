// setup_batch_interp.cpp -- test infrastructure: what the set-up kernel's batched load and write-out phases read from the host (csrc/plan.hpp build_at_map,
// oc_setup_tables; csrc/select.hpp SetupShape), for the pattern's handle as the library's own selection makes it (select_kernel with the knobs of the
// environment).  Host only.  tests/test_setup_batch_host.py checks the A' -> A map; tests/test_gpu_setup_batch.py reads the set-up shape.
#include <algorithm>
#include <vector>
#include "../../optimal_control_problem_amd/csrc/plan.hpp"
#include "../../optimal_control_problem_amd/csrc/select.hpp"

using namespace mpcqp;

// info: {two-kernel form, SetupShape.a_lds, .p_lds, .ix16, .batch, .at_map, the device array's header slot 8 (offset of the map in ints, 0 = none), nblk,
//        entries of A, entries of A', AT_MAP_NONE, the bits mpcqp.hip puts into DevOc.su_path}
// buf:   A.src, At.src, the map as the kernel reads it out of the device array (16 bits each, widened), each as {length, values ...}; returns the ints
//        written, or -(error) / -100 when cap is too small
extern "C" long setup_batch_describe(int n, int m, int batch, const int *Pp, const int *Pi, const int *Ap, const int *Ai, int cus, const char *forced_family, long *info, int *buf, long cap) {
  const Selection s = select_kernel(n, m, batch, Pp, Pi, Ap, Ai, cus, forced_family, Knobs::from_env());
  if (s.err) return -s.err;
  const Plan &pl = s.plan; const SetupShape &su = s.setup;
  const std::vector<int> tables = oc_setup_tables(pl, s.tlds, s.sing, s.at_map);
  const int o_map = tables[8 * (size_t)pl.nblk + 8];
  const int su_path = setup_path_bits(s);
  const long v[12] = {s.split, su.a_lds, su.p_lds, su.ix16, su.batch, su.at_map, o_map, pl.nblk, pl.A.entries(), pl.At.entries(), AT_MAP_NONE, su_path};
  std::copy(v, v + 12, info);
  std::vector<int> map;
  if (o_map > 0) {
    const unsigned short *p = reinterpret_cast<const unsigned short *>(tables.data() + o_map);
    map.assign(p, p + pl.At.entries());
  }
  const std::vector<int> *arr[] = {&pl.A.src, &pl.At.src, &map};
  long w = 0;
  for (const std::vector<int> *a : arr) {
    if (w + 1 + (long)a->size() > cap) return -100;
    buf[w++] = (int)a->size();
    std::copy(a->begin(), a->end(), buf + w); w += (long)a->size();
  }
  return w;
}
