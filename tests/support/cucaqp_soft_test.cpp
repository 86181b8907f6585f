// The C++ CuCaQP facade's setSoftRows (cpp/CuCaQP.hpp): one batch of QPs solved with hard rows, with soft rows, and with the weights cleared again.
// usage: cucaqp_soft_test <file>      file: int32 n, m, B, nnzP, nnzA, Pp[n + 1], Pi[nnzP], Ap[n + 1], Ai[nnzA], then the doubles
//                                     P[B nnzP], q[B n], A[B nnzA], l[B m], u[B m], w1[m], w2[m]
// prints, per step, "<hard|soft|cleared> status ..." / "... x ..." (hex floats: the test compares bits)
// Exit code 0 = ran, 3 = no GPU (the facade reported it as the reference would), 2 = bad file, 1 = a call failed.
#include <cstdio>
#include <vector>

#include "CuCaQP.hpp"

template <class T>
static bool rd(std::FILE *f, std::vector<T> &v, size_t count) { v.resize(count); return count == 0 || std::fread(v.data(), sizeof(T), count, f) == count; }

static void show(const char *step, const CuCaQP &qp) {
  std::printf("%s status", step); for (int s : qp.getStatus()) std::printf(" %d", s);
  std::printf("\n%s x", step); for (double v : qp.getSolutionVector()) std::printf(" %a", v);
  std::printf("\n");
}

int main(int argc, char **argv) {
  if (argc < 2) {      // (no file: the program was built and the facade refuses what it must)
    CuCaQP qp;
    qp.setSoftRows(nullptr);
    return qp.solve() ? 1 : 3;
  }
  std::FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<int> hd, Pp, Pi, Ap, Ai;
  if (!rd(f, hd, 5)) return 2;
  const int n = hd[0], m = hd[1], B = hd[2], nnzP = hd[3], nnzA = hd[4];
  if (!rd(f, Pp, n + 1) || !rd(f, Pi, nnzP) || !rd(f, Ap, n + 1) || !rd(f, Ai, nnzA)) return 2;
  std::vector<double> P, q, A, l, u, w1, w2;
  if (!rd(f, P, (size_t)B * nnzP) || !rd(f, q, (size_t)B * n) || !rd(f, A, (size_t)B * nnzA) || !rd(f, l, (size_t)B * m) || !rd(f, u, (size_t)B * m) || !rd(f, w1, m) || !rd(f, w2, m)) return 2;
  std::fclose(f);
  CuCaQP qp(B);
  if (!qp.setDimension(n, m)) return 1;
  qp.setSystem({n, n, Pp.data(), Pi.data(), P.data()}, q.data(), {m, n, Ap.data(), Ai.data(), A.data()}, l.data(), u.data());
  if (!qp.initSolver()) return 3;
  if (!qp.solve()) return 1;
  show("hard", qp);
  qp.setSoftRows(w1.data(), w2.data());
  if (!qp.solve()) return 1;
  show("soft", qp);
  qp.setSoftRows(nullptr);
  if (!qp.solve()) return 1;
  show("cleared", qp);
  return 0;
}
