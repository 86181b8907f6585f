"""Batches, tiling and launch arithmetic shared by tests/test_batch_geometry_host.py (CPU) and tests/test_gpu_batch_geometry.py -- TEST
INFRASTRUCTURE ONLY.

The NLP-side kernels are pinned to their references at the batches of their case tables (2 to 7 instances).  Here the same cases are launched at
batches that cross every launch boundary: `tile` gathers a base case to any batch, `threads` restates how a launch of that batch is cut into
threads, groups and blocks (from the comments and launchers of csrc/stage_kernels.hpp, csrc/stage_eval.hip and csrc/general_kernels.hpp, not from
running them), and JOBS lists which operation runs on which case."""
import collections
import functools

import numpy as np

from optimal_control_problem_amd import general_eval, models
from tests.support import convexify_cases as cc
from tests.support import exact_hessian_cases as ec
from tests.support import general_exact_hessian_cases as ge
from tests.support import general_linesearch_cases as gl
from tests.support import hp_cases as hc
from tests.support import residual_cases as rc

# 4 | 5: the kernels with one wave per instance and four per block get their second block; 63 | 64 | 65: one wave of threads with an instance each;
# 257: the second block of the kernels with one thread per instance; 1031: prime, more than four blocks of every kernel, the last one partial
BATCHES = (1, 4, 5, 63, 64, 65, 257, 1031)
SEQUENCE = (5, 1031, 64, 1, 257)                    # one handle: grow, shrink, shrink, grow below the capacity
PER_INSTANCE = ("p", "x", "lbx", "ubx", "lbg", "ubg", "status", "theta", "plant", "d", "d_new", "w", "s_meas", "q", "dw", "y", "mu", "hnorm")
NO_POINT = (3, 9, 11)
GL_MU0 = np.array([0.0, 50.0, 0.5, 7.0, 0.0, 3.0, 1e4])      # the penalties of tests/test_gpu_general_linesearch.py


# ------------------------------------------------------------------------------------------------ tiling
def index(B, B0):
    """idx [B]: instance b of a tiled case is base instance idx[b] = (7 b + 3) mod B0.  Two corrections keep the property the formula is chosen
    for -- every base instance in each of the four wave slots b mod 4 of a block -- at the base batches where it would lose it: with seven base
    instances 7 b mod 7 is constant, so those cases step by 5; with an even number 4 * 7 t mod B0 never changes parity along a slot, so b // 4 is
    added.  A slot of a batch B holds B / 4 instances: the property needs B >= 4 B0."""
    b = np.arange(B)
    step = 7 if B0 % 7 else 5
    return (step * b + 3 + (b // 4 if B0 % 2 == 0 else 0)) % B0


def tile(case, B):
    """(the case at batch B, idx [B]): every per-instance array gathered by idx = index(B, B0); model, name and the rest are shared"""
    B0 = case["x"].shape[0]
    idx = index(B, B0)
    out = dict(case)
    for k in PER_INSTANCE:
        v = case.get(k)
        if v is not None:
            assert v.shape[0] == B0, (case["name"], k, v.shape)
            out[k] = np.ascontiguousarray(v[idx])
    return out, idx


# ------------------------------------------------------------------------------------------------ base cases
@functools.lru_cache(maxsize=None)
def base(family, name):
    """the existing case `name` of a table as one dict: model and the per-instance arrays of PER_INSTANCE (None where the case has none).  Built once
    and left unchanged; callers copy what they change."""
    c = dict.fromkeys(PER_INSTANCE)
    if family == "hp":                                 # tests/support/hp_cases.py: the zoo, the generated models, the convexify cases
        h = hc.case(name)
        c.update({k: h[k] for k in h if k in PER_INSTANCE}, model=h["model"], kind=h["kind"])
        if h["kind"] == "convexify":
            c["hnorm"] = cc.case(name)["hnorm"]
        else:
            c["q"], c["dw"], c["y"] = hc.step(name)
            c["mu"] = hc.MU0.copy()
        if c["d"] is not None:
            c["d_new"] = np.random.default_rng(5).normal(0.5, 0.2, size=(c["x"].shape[0], c["model"].nsd))
    elif family == "exact":                            # tests/support/exact_hessian_cases.py
        e = ec.case(name)
        c.update({k: e[k] for k in e if k in PER_INSTANCE}, model=e["model"], kind="exact")
    elif family == "gn":                               # tests/support/residual_cases.py
        r = rc.case(name)
        c.update(r["pt"], model=r["model"], kind="gn")
    elif family == "general":                          # hp_cases.GENERAL; the step is this module's: a drawn dw, instance 1 without a point
        g = hc.general_case(name)
        c.update({k: g[k] for k in g if k in PER_INSTANCE}, model=g["model"], kind="general")
        c["dw"] = np.random.default_rng(6).normal(0.0, 0.3, size=(g["x"].shape[0], g["model"].n))
        c["status"] = np.array([1, 3, 7], np.int32)
    elif family == "gls":                              # tests/support/general_linesearch_cases.py, the arrangement with the statuses 3, 9 and 11
        k = gl.kernel_case(name)
        c.update({v: k[v] for v in ("p", "x", "lbx", "ubx", "lbg", "ubg", "q")}, model=k["model"], kind="gls", mu=GL_MU0.copy())
        c["dw"], c["y"], c["status"] = gl.arrangement(k, 0)
    elif family == "gexact":                           # tests/support/general_exact_hessian_cases.py: NaN multipliers where the QP failed
        g = ge.case(name)
        c.update({k: g[k] for k in ("p", "x", "lbx", "ubx", "lbg", "ubg", "status")}, model=g["model"], kind="gexact", y=g["ynan"])
    else:
        raise KeyError(family)
    c.update(name=name, family=family)
    return c


# ------------------------------------------------------------------------------------------------ what runs where
Job = collections.namedtuple("Job", "family name op kw")
STAGE_KERNEL = {"eval": "stage_eval", "merit": "stage_merit", "step": "stage_step", "linesearch": "stage_linesearch", "advance": "stage_advance",
                "convexify": "stage_convexify", "lagrangian": "stage_lagrangian", "shift_data": "stage_shift_data"}
GENERAL_KERNEL = {"nlp_eval": "general_eval", "nlp_merit": "general_merit", "nlp_step": "general_step", "nlp_linesearch": "general_linesearch",
                  "nlp_lagrangian": "general_lagrangian"}
KERNEL = dict(STAGE_KERNEL, **GENERAL_KERNEL)

ZOO = ("cartpole3", "quadrotor2", "quadrotor2_pfw", "di2_pfw")       # f = 5: the plain mapping; the cooperative one without and with the padded group
GENERATED = ("every3", "every_pf4", "link_quadrotor")
CONVEXIFY = ("bump3", "quad_dense", "wide")                          # nl = 9, 28, 33: the group widths 16, 32 and 64
EXACT = (("pend_theta_sd", None), ("cvx", "project"), ("wide7", "mirror"))
GAUSS_NEWTON = ("tip_pf", "cart_wide", "quad_tilt")
GLS_CANDIDATES = (1, 3, 7, 8)                                        # the group widths 2, 4, 8 and 16


def _jobs():
    out = []
    for name in ZOO + GENERATED:
        out += [Job("hp", name, op, ()) for op in ("eval", "merit", "step", "linesearch")]
        if name in hc.ADVANCE:
            out.append(Job("hp", name, "advance", ()))
        if name in hc.EVERY:
            out += [Job("hp", name, "convexify", (("mode", m),)) for m in hc.MODES]
    out += [Job("hp", "data70", op, ()) for op in ("merit", "linesearch")]
    out += [Job("hp", name, "convexify", (("mode", m),)) for name in CONVEXIFY for m in hc.MODES]
    out += [Job("exact", name, "lagrangian", (("mode", m),)) for name, m in EXACT]
    out += [Job("gn", name, op, ()) for name in GAUSS_NEWTON for op in ("eval", "merit")]
    out += [Job("general", name, op, ()) for name in hc.GENERAL for op in ("nlp_eval", "nlp_merit", "nlp_step")]
    out += [Job("gls", "pendulum", "nlp_linesearch", (("candidates", K),)) for K in GLS_CANDIDATES]
    out += [Job("gexact", name, "nlp_lagrangian", kw) for name in ge.NAMES for kw in ((("mode", 0), ("workspace", False)), (("mode", "dominant"), ("workspace", True)))]
    return tuple(out)


JOBS = _jobs()


def job_id(j):
    return "-".join([j.family, j.name, j.op] + [str(v) for _, v in j.kw])


# ------------------------------------------------------------------------------------------------ the launch arithmetic
# one block range of a launch: `per` threads per instance (consecutive, instance-major), `block` threads per block, `blocks` launched
Range = collections.namedtuple("Range", "name per block blocks")


def _range(name, per, block, B):
    return Range(name, per, block, -(-B * per // block))


def is_zoo(model):
    """the built-in functor runs this model (stage_eval.StageEvaluator's rule): a zoo class with its own dynamics and nothing generated"""
    for cls in (models.DoubleIntegrator, models.Quadrotor, models.CartPole):
        if isinstance(model, cls) and model.name == cls.name and type(model).F is cls.F and type(model).cdyn is cls.cdyn:
            return not (model.nh > 0 or model.nk > 0 or model.general_cost or model.link_cost)
    return False


def convexify_groups(model):
    """(nl, W, G) of stage_cvx: the tile's order, the lanes of a group, the groups of a block (two nl x nl tiles per group in 48 KiB, at most 4 waves)"""
    nl = 2 * model.nx + model.nu
    W = 16 if nl <= 16 else 32 if nl <= 32 else 64
    fit, per_wave = (48 * 1024) // (2 * nl * nl * 8), 64 // W
    waves = 4 if fit // per_wave >= 4 else max(fit // per_wave, 1)
    return nl, W, waves * per_wave


def line_search_width(candidates):
    """gn_ls_group_width: the lanes of an instance's group"""
    return 2 if candidates + 1 <= 2 else 4 if candidates + 1 <= 4 else 8 if candidates + 1 <= 8 else 16


def threads(kernel, model, B, mode=None, candidates=None, workspace=False):
    """the block ranges of one launch of `kernel` at batch B, in launch order: a list of Range"""
    wave = lambda name: [_range(name, 64, 256, B)]                   # one wave per instance, four per block
    if kernel in ("stage_merit", "stage_advance", "stage_linesearch", "stage_step", "general_step"):
        return wave(kernel)
    if kernel == "stage_eval":
        # one thread per column of [p; x]; the cooperative functor (the zoo quadrotor, f = 16 divides 64): f slots per frame behind the parameter
        # group, which is f slots (a shared reference) or ceil(N nx / f) f (per-frame references), the padding lanes leaving early
        N, nx, f = model.N, model.nx, model.f
        coop = is_zoo(model) and isinstance(model, models.Quadrotor) and 64 % f == 0
        ppad = -(-N * nx // f) * f if model.pref else f
        return [_range("columns", ppad + f * N if coop else model.n, 256, B)]
    if kernel == "stage_convexify":
        _, W, G = convexify_groups(model)                            # a group of W lanes per (instance, frame), G groups per block
        return [_range("tiles", model.N * W, G * W, B), _range("sum", model.nx * model.nx, 256, B)]
    if kernel == "stage_lagrangian":
        add = [_range("columns", model.N * model.f, 256, B)]         # one thread per (instance, frame, column of [s; u])
        return add + (threads("stage_convexify", model, B) if mode else [])
    if kernel == "stage_shift_data":
        return [_range("elements", model.N * model.nsd, 256, B)]
    if kernel == "general_merit":
        return [_range("instances", 1, 256, B)]
    if kernel == "general_linesearch":
        return [_range("groups", line_search_width(candidates), 256, B)]
    comp = general_eval.compress(model)
    if kernel == "general_eval":                                     # three block ranges of one launch
        return [_range("hessian", comp["hp"], 256, B), _range("jacobian", comp["jp"], 256, B), _range("identity", model.n, 256, B)]
    if kernel == "general_lagrangian":                               # one thread per (instance, pass), then per (instance, column with curvature)
        if comp["cp"] == 0:
            return []
        return [_range("curvature", comp["cp"], 256, B)] + ([_range("apply", len(comp["ccols"]), 256, B)] if workspace else [])
    raise KeyError(kernel)


def job_threads(j, B):
    return threads(KERNEL[j.op], base(j.family, j.name)["model"], B, **dict(j.kw))


def can_straddle(r):
    """an instance's threads can lie across a block boundary: its thread count does not divide the block's"""
    return r.per > 0 and r.block % r.per != 0


def straddlers(r, B):
    """the instances of a batch B whose threads lie in more than one block of the range"""
    b = np.arange(B)
    return b[(b * r.per) // r.block != ((b + 1) * r.per - 1) // r.block] if r.per > 0 else b[:0]


def last_block_partial(r, B):
    return (B * r.per) % r.block != 0


def probe_rows(j, B):
    """three rows of a launch at batch B: the first, the last and one whose threads lie across a block boundary (where the mapping has none: one in
    the middle of the batch)"""
    mid = B // 2
    for r in job_threads(j, B):
        s = straddlers(r, B)
        if len(s):
            mid = int(s[len(s) // 2])
            break
    return np.array([0, mid, B - 1])
