// The C++ CuCaQP facade's setKeepScaling (cpp/CuCaQP.hpp) on a batch read from a file: setSystem(QP1) -> initSolver -> solve, then
// updateHessianMatrix / updateLinearConstraintsMatrix / updateGradient / updateLowerBound / updateUpperBound with QP2 -> solve, once with
// setKeepScaling(true) (mpcqp_update_matrices: the scaling of QP1 stays) and once without (a full set-up), each on its own object.
// usage: cucaqp_keep_scaling_test <file>      file: int32 n, m, B, nnzP, nnzA, Pp[n + 1], Pi[nnzP], Ap[n + 1], Ai[nnzA], then for QP1 and QP2 the doubles
//                                             P[B nnzP], q[B n], A[B nnzA], l[B m], u[B m]
// prints, per run, "keep <0|1> status ..." / "keep <0|1> iters ..." / "keep <0|1> x ..." (hex floats: the test compares bits)
// Exit code 0 = ran, 3 = no GPU (the facade reported it as the reference would), 2 = bad file, 1 = a call failed.
#include <cstdio>
#include <vector>

#include "CuCaQP.hpp"

struct QP { std::vector<double> P, q, A, l, u; };

template <class T>
static bool rd(std::FILE *f, std::vector<T> &v, size_t count) { v.resize(count); return count == 0 || std::fread(v.data(), sizeof(T), count, f) == count; }

int main(int argc, char **argv) {
  if (argc < 2) {      // (no file: the program was built and the facade refuses what it must)
    CuCaQP qp;
    qp.setKeepScaling(true);
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
  for (int keep = 1; keep >= 0; keep--) {
    CuCaQP qp(B);
    if (!qp.setDimension(n, m)) return 1;
    const QP &a = qps[0], &b = qps[1];
    qp.setSystem({n, n, Pp.data(), Pi.data(), a.P.data()}, a.q.data(), {m, n, Ap.data(), Ai.data(), a.A.data()}, a.l.data(), a.u.data());
    if (!qp.initSolver()) return 3;
    if (!qp.solve()) return 1;
    qp.setKeepScaling(keep != 0);
    if (!qp.updateHessianMatrix({n, n, Pp.data(), Pi.data(), b.P.data()}) || !qp.updateLinearConstraintsMatrix({m, n, Ap.data(), Ai.data(), b.A.data()}) ||
        !qp.updateGradient(b.q.data(), n) || !qp.updateLowerBound(b.l.data(), m) || !qp.updateUpperBound(b.u.data(), m) || !qp.solve()) return 1;
    std::printf("keep %d status", keep); for (int s : qp.getStatus()) std::printf(" %d", s);
    std::printf("\nkeep %d iters", keep); for (int s : qp.getIterations()) std::printf(" %d", s);
    std::printf("\nkeep %d x", keep); for (double v : qp.getSolutionVector()) std::printf(" %a", v);
    std::printf("\n");
  }
  return 0;
}
