/* A plain C client of the hand-over between two MPC ticks (include/mpcqp.h, mpcqp_stage_advance): create a double-integrator evaluator with
 * three frames, put a trajectory, bounds, a QP start and duals on the device, advance once per tail, print what comes back.  The test compares
 * the printed numbers with the NumPy statement (models.StageOCP.advance).  Exit codes: 0 ok, 3 refused for lack of a GPU (after the host-only
 * checks passed), anything else a failure. */
#include <stdio.h>
#include <string.h>

#include <hip/hip_runtime_api.h>

#include "mpcqp.h"

#define NF 3
#define NX 2
#define NU 1
#define F (NX + NU)
#define B 2
#define NV (NF * F)
#define NN (NX + NV)
#define NM (NN + (NF - 1) * NX)

static double *up(const double *h, size_t cnt) {
  double *d = NULL;
  if (hipMalloc((void **)&d, cnt * sizeof(double)) != hipSuccess || hipMemcpy(d, h, cnt * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) return NULL;
  return d;
}

static void show(const char *tag, int tail, const double *d, int w) {
  static double h[B * NM];
  if (hipMemcpy(h, d, sizeof(double) * B * w, hipMemcpyDeviceToHost) != hipSuccess) { printf("copy failed\n"); return; }
  for (int b = 0; b < B; b++) {
    printf("%s %d %d", tag, tail, b);
    for (int i = 0; i < w; i++) printf(" %.17g", h[b * w + i]);
    printf("\n");
  }
}

int main(void) {
  mpcqp_stage_desc d;
  if (mpcqp_stage_default(MPCQP_MODEL_DOUBLE_INTEGRATOR, NF, &d) != MPCQP_OK) return 1;
  d.dt = 0.5;
  mpcqp_stage_advance_args a;
  memset(&a, 0, sizeof a);
  if (mpcqp_stage_advance(NULL, B, &a, NULL) != MPCQP_ERR_ARG) { fprintf(stderr, "a null handle was not refused\n"); return 1; }
  printf("host checks ok\n");
  mpcqp_stage *s = NULL;
  int rc = mpcqp_stage_create(&d, &s);
  if (rc == MPCQP_ERR_NO_GPU) { fprintf(stderr, "refused: %s\n", mpcqp_strerror(rc)); return 3; }
  if (rc != MPCQP_OK) { fprintf(stderr, "create: %s\n", mpcqp_strerror(rc)); return 1; }
  const double x[B * NV] = {1.0, 2.0, 4.0, 3.0, 4.0, 8.0, 5.0, 6.0, -8.0, 0.0, -2.0, 0.0, -1.0, 0.0, 2.0, 10.0, 0.0, 4.0};
  double lb[B * NV], ub[B * NV], dw[B * NN], y[B * NM], zero[B * NM];
  const int status[B] = {MPCQP_SOLVED, 3};
  for (int i = 0; i < B * NV; i++) { lb[i] = -100.0 + i; ub[i] = 100.0 + i; }
  for (int i = 0; i < B * NN; i++) dw[i] = 0.5 + i;
  for (int i = 0; i < B * NM; i++) { y[i] = -0.25 * i; zero[i] = 0.0; }
  int *dst = NULL;
  if (hipMalloc((void **)&dst, sizeof status) != hipSuccess || hipMemcpy(dst, status, sizeof status, hipMemcpyHostToDevice) != hipSuccess) return 1;
  for (int tail = MPCQP_TAIL_REPEAT; tail <= MPCQP_TAIL_ROLLOUT; tail++) {
    double *dx = up(x, B * NV), *dxo = up(zero, B * NV), *dlb = up(lb, B * NV), *dub = up(ub, B * NV), *ddw = up(dw, B * NN), *ddwo = up(zero, B * NN),
           *dy = up(y, B * NM), *dyo = up(zero, B * NM);
    if (!dx || !dxo || !dlb || !dub || !ddw || !ddwo || !dy || !dyo) { fprintf(stderr, "device memory\n"); return 1; }
    memset(&a, 0, sizeof a);
    a.x_in = dx; a.x_out = dxo; a.lbx = dlb; a.ubx = dub; a.status = dst; a.dw_in = ddw; a.dw_out = ddwo; a.y_in = dy; a.y_out = dyo; a.tail = tail;
    if ((rc = mpcqp_stage_advance(s, B, &a, NULL)) != MPCQP_OK || hipDeviceSynchronize() != hipSuccess) { fprintf(stderr, "advance: %s\n", mpcqp_strerror(rc)); return 1; }
    show("x", tail, dxo, NV); show("lbx", tail, dlb, NV); show("ubx", tail, dub, NV); show("dw", tail, ddwo, NN); show("y", tail, dyo, NM);
    hipFree(dx); hipFree(dxo); hipFree(dlb); hipFree(dub); hipFree(ddw); hipFree(ddwo); hipFree(dy); hipFree(dyo);
  }
  hipFree(dst);
  mpcqp_stage_destroy(s);
  printf("advance from C ok\n");
  return 0;
}
