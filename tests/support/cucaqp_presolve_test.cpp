// The C++ CuCaQP facade's setPresolveFixedRows (cpp/CuCaQP.hpp) when a later system unpins a row: setSystem(QP1) -> initSolver -> solve, then QP2 -- the
// same QP with other bounds -- once through setSystem -> initSolver -> solve ("system") and once through updateLowerBound / updateUpperBound -> solve
// ("updates"), each on its own object.  A presolved handle eliminates the rows that were pinned when it was created; the facade has to notice that QP2 pins
// another set and build a new handle instead of answering MPCQP_UNSOLVED / NaN.
// usage: cucaqp_presolve_test <file>      file: int32 n, m, B, nnzP, nnzA, Pp[n + 1], Pi[nnzP], Ap[n + 1], Ai[nnzA], then for QP1 and QP2 the doubles
//                                         P[B nnzP], q[B n], A[B nnzA], l[B m], u[B m]
// prints, per mode and step, "<mode> <1|2> nfixed N" / "... status ..." / "... x ..." (hex floats: the test compares bits)
// Exit code 0 = ran, 3 = no GPU (the facade reported it as the reference would), 2 = bad file, 1 = a call failed.
#include <cstdio>
#include <vector>

#include "CuCaQP.hpp"

struct QP { std::vector<double> P, q, A, l, u; };

template <class T>
static bool rd(std::FILE *f, std::vector<T> &v, size_t count) { v.resize(count); return count == 0 || std::fread(v.data(), sizeof(T), count, f) == count; }

static void show(const char *mode, int step, const CuCaQP &qp) {
  std::printf("%s %d nfixed %d\n", mode, step, qp.presolvedRows());
  std::printf("%s %d status", mode, step); for (int s : qp.getStatus()) std::printf(" %d", s);
  std::printf("\n%s %d x", mode, step); for (double v : qp.getSolutionVector()) std::printf(" %a", v);
  std::printf("\n");
}

int main(int argc, char **argv) {
  if (argc < 2) {      // (no file: the program was built and the facade refuses what it must)
    CuCaQP qp;
    qp.setPresolveFixedRows(true);
    return qp.solve() ? 1 : 3;
  }
  std::FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<int> hd, Pp, Pi, Ap, Ai;
  if (!rd(f, hd, 5)) return 2;
  const int n = hd[0], m = hd[1], B = hd[2], nnzP = hd[3], nnzA = hd[4];
  if (!rd(f, Pp, n + 1) || !rd(f, Pi, nnzP) || !rd(f, Ap, n + 1) || !rd(f, Ai, nnzA)) return 2;
  QP qps[2];
  for (QP &d : qps)
    if (!rd(f, d.P, (size_t)B * nnzP) || !rd(f, d.q, (size_t)B * n) || !rd(f, d.A, (size_t)B * nnzA) || !rd(f, d.l, (size_t)B * m) || !rd(f, d.u, (size_t)B * m)) return 2;
  std::fclose(f);
  const QP &a = qps[0], &b = qps[1];
  for (int updates = 0; updates < 2; updates++) {
    const char *mode = updates ? "updates" : "system";
    CuCaQP qp(B);
    qp.setPresolveFixedRows(true);
    if (!qp.setDimension(n, m)) return 1;
    qp.setSystem({n, n, Pp.data(), Pi.data(), a.P.data()}, a.q.data(), {m, n, Ap.data(), Ai.data(), a.A.data()}, a.l.data(), a.u.data());
    if (!qp.initSolver()) return 3;
    if (!qp.solve()) return 1;
    show(mode, 1, qp);
    if (updates) {
      if (!qp.updateLowerBound(b.l.data(), m) || !qp.updateUpperBound(b.u.data(), m)) return 1;
    } else {
      qp.setSystem({n, n, Pp.data(), Pi.data(), b.P.data()}, b.q.data(), {m, n, Ap.data(), Ai.data(), b.A.data()}, b.l.data(), b.u.data());
      if (!qp.initSolver()) return 1;
    }
    if (!qp.solve()) return 1;
    show(mode, 2, qp);
  }
  return 0;
}
