"""CPU: what the set-up kernel's factorisation reads on chip (csrc/plan.hpp build_t_lds_plan, build_sing_list, oc_setup_tables), for the
handles the library's own selection makes of the MPC patterns (tests/support/t_lds_interp.cpp): the parts of the T tiles in LDS, the singleton list
of the diagonal term, the array the kernel reads them from, and a NumPy re-assembly of M = P + sigma I + A' rho A from the per-part tables alone."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from optimal_control_problem_amd import models
from tests.support import problems

SO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "support", "libt_lds_interp.so")
CUS = problems.selection_grid()["multiProcessorCount"]
BS, BLK, WAVE = 16, 256, 64
INFO = ["split", "lds_bytes", "stage", "t_parts", "sing_k", "fit_parts", "cap", "rec_off", "nblk", "nT", "npad", "mpad", "n", "m", "nb", "max_parts", "vecs", "tabw"]
ARRAYS = ["blk0", "image", "sc_ptr", "sc", "rec", "ta", "tb", "tiles_ptr", "tiles", "tpos", "asm_ptr", "asm_a", "asm_b", "blk_diag", "asm_pidx", "blkI", "blkJ",
          "pos", "perm", "A_off", "A_src", "At_off", "At_src", "At_idx", "At_flag", "P_src", "sing_ent", "sing_row", "tables"]
# id -> (workload, N, reduced, parts the rule gives on 256 CUs: pinned; 0 = the slab path)
CASES = {
    "quadrotor-N20": ("quadrotor", 20, False, 3),             # the north star: A's values staged at three workgroups per CU, 18 tiles of room
    "quadrotor-N50": ("quadrotor", 50, False, 0),             # nothing staged: room for a dozen tiles, more parts than the rule takes
    "cartpole-N30": ("cartpole", 30, False, 2),               # four waves, two pairs of chains
    "cartpole-N100": ("cartpole", 100, False, 0),            # nothing staged either: ten tiles of room for 63
    "double_integrator-N60": ("double_integrator", 60, False, 2),
    "quadrotor-N20-reduced": ("quadrotor", 20, True, 3),      # no arrow head
}


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@functools.lru_cache(maxsize=None)
def _system(name, N, reduced):
    mdl, ls, _ = models.make_workload(name, 2, N=N)
    return problems.reduce_qp(ls, list(range(mdl.np)))[0] if reduced else ls


def _describe(ls, env=()):
    L = C.CDLL(SO)
    L.t_lds_describe.restype = C.c_long
    info = np.zeros(len(INFO), np.int64); buf = np.zeros(1 << 22, np.int32)
    Pp, Pi, Ap, Ai = (np.ascontiguousarray(a, dtype=np.int32) for a in (ls.Pp, ls.Pi, ls.Ap, ls.Ai))
    old = {k: os.environ.get(k) for k, _ in env}
    try:
        for k, v in env:
            os.environ[k] = v
        w = L.t_lds_describe(ls.n, ls.m, 8192, _p(Pp), _p(Pi), _p(Ap), _p(Ai), CUS, None, _p(info), _p(buf), C.c_long(buf.size))
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    assert w > 0, w
    arrays, o = {}, 0
    for name in ARRAYS:
        cnt = int(buf[o]); arrays[name] = buf[o + 1:o + 1 + cnt].copy(); o += 1 + cnt
    assert o == w
    return dict(zip(INFO, info.tolist())), arrays


@functools.lru_cache(maxsize=None)
def _case(cid):
    name, N, reduced, _ = CASES[cid]
    return _describe(_system(name, N, reduced))


def _off(r, c):
    """plan.hpp t_lds_off"""
    s = r >> 1
    return r * BS + ((((c >> 1) ^ s ^ (((s + 2) >> 1) & 2)) << 1) | (c & 1))


def test_image_layout_is_a_permutation_of_the_tile_and_free_of_bank_conflicts(built):
    L = C.CDLL(SO)
    offs = np.array([[L.t_lds_off_host(r, c) for c in range(BS)] for r in range(BS)])
    assert np.array_equal(offs, np.array([[_off(r, c) for c in range(BS)] for r in range(BS)]))
    assert sorted(offs.ravel().tolist()) == list(range(BLK))
    assert (offs // BS == np.arange(BS)[:, None]).all()                   # an element stays in its row
    assert (offs[:, 0::2] % 2 == 0).all() and (offs[:, 1::2] == offs[:, 0::2] + 1).all()      # 16-byte pairs stay whole: the row piece is two ds_read_b128
    # the four lane groups of ds_read_b128: sixteen different 16-byte slots of the 256-byte bank row each, for either half of the row piece
    groups = [list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)), list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32))]
    groups += [[l + 32 for l in g] for g in groups]
    for half in (0, 2):
        for g in groups:
            slots = {(8 * offs[l & 15, 4 * (l >> 4) + half] // 16) % 16 for l in g}
            assert len(slots) == 16


@pytest.mark.parametrize("cid", CASES)
def test_parts_cover_the_blocks_and_fit(built, cid):
    info, a = _case(cid)
    assert info["split"] == 1
    # the fit function and the selection agree, and the rule gives what is pinned here
    assert info["t_parts"] == info["fit_parts"] == CASES[cid][3]
    # never a reason to ask for more LDS: the records sit behind the images inside the block-slot region and x
    assert info["lds_bytes"] >= 8 * (info["stage"] + info["npad"])
    if cid == "quadrotor-N20":
        assert 3 * info["lds_bytes"] <= 160 * 1024          # three set-up workgroups per CU, as before
    P = info["t_parts"]
    if P == 0:
        assert a["blk0"].size == 0 and a["sc"].size == 0
        return
    assert 0 < P <= info["max_parts"]
    assert info["rec_off"] == info["stage"] + info["npad"] - 4 * info["nblk"] and info["cap"] == info["rec_off"] // BLK * BLK
    blk0 = a["blk0"]
    assert blk0[0] == 0 and blk0[-1] == info["nblk"] and (np.diff(blk0) > 0).all() and blk0.size == P + 1
    for p in range(P):
        tiles = a["tiles"][a["tiles_ptr"][p]:a["tiles_ptr"][p + 1]]
        assert len(set(tiles.tolist())) == tiles.size and a["image"][p] == (1 + tiles.size) * BLK <= info["cap"]
        slot = {int(t): k + 1 for k, t in enumerate(tiles)}
        used = set()
        for b in range(blk0[p], blk0[p + 1]):
            g0, g1 = a["asm_ptr"][b], a["asm_ptr"][b + 1]
            rec = a["rec"][8 * b:8 * b + 8]
            assert rec[0] == g1 - g0 and rec[1] == a["blk_diag"][b]
            for g in range(g0, g1):          # today's order of the terms; every term's tiles inside the part (the tail past the third too)
                assert a["ta"][g] == slot[int(a["asm_a"][g])] and a["tb"][g] == slot[int(a["asm_b"][g])]
                used |= {int(a["asm_a"][g]), int(a["asm_b"][g])}
            for t in range(3):
                want = (a["ta"][g0 + t], a["tb"][g0 + t]) if t < g1 - g0 else (0, 0)       # (unused terms: the zero tile in slot 0)
                assert (rec[2 + 2 * t], rec[3 + 2 * t]) == want
        assert used == set(slot)             # no tile scattered that no block of the part multiplies
        # every entry of A with a place in one of the part's tiles is scattered, once, to its place in the image, and nothing else is
        sc = a["sc"][2 * a["sc_ptr"][p]:2 * a["sc_ptr"][p + 1]].reshape(-1, 2)
        ent, packed = sc[:, 0], sc[:, 1].astype(np.int64) & 0xffffffff
        tq = a["tpos"]
        want = np.flatnonzero((tq >= 0) & np.isin(tq // BLK, tiles))
        assert np.array_equal(ent, want)
        rows = np.repeat(np.arange(a["A_off"].size - 1), np.diff(a["A_off"]) * WAVE) * WAVE + np.tile(np.arange(WAVE), a["A_off"][-1])
        assert np.array_equal(packed >> 16, rows[ent])
        off = np.array([slot[int(t) // BLK] * BLK + _off((int(t) % BLK) // BS, int(t) % BS) for t in tq[ent]])
        assert np.array_equal(packed & 0xffff, off) and off.max() < a["image"][p] and len(set(off.tolist())) == off.size


@pytest.mark.parametrize("cid", CASES)
def test_singleton_list_is_the_flagged_entries_in_slot_order(built, cid):
    info, a = _case(cid)
    K, npad = info["sing_k"], info["npad"]
    assert K % 2 == 0 and a["sing_ent"].size == K * npad == a["sing_row"].size
    ent = a["sing_ent"].reshape(K, npad); row = a["sing_row"].reshape(K, npad)
    flagged = np.flatnonzero(a["At_flag"])
    assert sorted(ent[ent >= 0].tolist()) == flagged.tolist()
    most = 0
    for t in range(npad):
        e = ent[:, t]; k = int((e >= 0).sum()); most = max(most, k)
        assert (e[:k] >= 0).all() and (e[k:] == -1).all() and (row[k:, t] == -1).all()
        assert (e[:k] % WAVE == t % WAVE).all() and (np.diff(e[:k]) > 0).all()          # this column's lane, ascending slots
        s = e[:k] // WAVE
        assert ((s >= a["At_off"][t // WAVE]) & (s < a["At_off"][t // WAVE + 1])).all()
        assert np.array_equal(row[:k, t], a["At_idx"][e[:k]])
    assert K == (most + 1) // 2 * 2


@pytest.mark.parametrize("cid", CASES)
def test_device_array_holds_the_tables_where_its_header_says(built, cid):
    info, a = _case(cid)
    t, h = a["tables"], 8 * info["nblk"]
    hd = t[h:h + 16]
    assert hd[0] == info["t_parts"] and hd[6] == info["sing_k"]
    K, npad = info["sing_k"], info["npad"]
    if K:
        assert hd[7] % 2 == 0 and np.array_equal(t[hd[7]:hd[7] + K * npad], a["sing_ent"]) and np.array_equal(t[hd[7] + K * npad:hd[7] + 2 * K * npad], a["sing_row"])
    if info["t_parts"]:
        assert hd[1] == info["rec_off"] and np.array_equal(t[hd[2]:hd[2] + h], a["rec"])
        assert np.array_equal(t[hd[3]:hd[3] + a["ta"].size], a["ta"]) and np.array_equal(t[hd[4]:hd[4] + a["tb"].size], a["tb"])
        for p in range(info["t_parts"]):
            b0, b1, img, o_sc, cnt = t[hd[5] + 8 * p:hd[5] + 8 * p + 5]
            assert (b0, b1, img) == (a["blk0"][p], a["blk0"][p + 1], a["image"][p]) and o_sc % 2 == 0
            assert np.array_equal(t[o_sc:o_sc + 2 * cnt], a["sc"][2 * a["sc_ptr"][p]:2 * a["sc_ptr"][p + 1]])
    else:       # the slab path's records: unused terms at the zero tile behind the T tiles
        assert (t[:h].reshape(-1, 8)[:, 0] >= 0).all()


def test_switches_turn_each_part_off(built):
    ls = _system("quadrotor", 20, False)
    assert _describe(ls, (("MPCQP_NO_T_LDS", "1"),))[0]["t_parts"] == 0 and _describe(ls, (("MPCQP_NO_T_LDS", "1"),))[0]["sing_k"] > 0
    assert _describe(ls, (("MPCQP_NO_SING_LIST", "1"),))[0]["sing_k"] == 0 and _describe(ls, (("MPCQP_NO_SING_LIST", "1"),))[0]["t_parts"] > 0


@pytest.mark.parametrize("cid", [c for c in CASES if CASES[c][3] > 0])
def test_reassembly_from_the_part_tables_is_the_dense_matrix(built, cid):
    """S_b = sum_g T_a(g) T_b(g)' + P entries + d on the diagonal, the tiles read from each part's image as the kernel reads them, against the
    dense P + sigma I + A' diag(rho) A in the plan's positions (1 on the diagonal of a padding position) to 1e-13 of the largest entry"""
    name, N, reduced, _ = CASES[cid]
    ls = _system(name, N, reduced); info, a = _case(cid)
    rng = np.random.default_rng(3)
    Av = rng.normal(size=ls.Ai.size); rho = rng.choice([0.1, 100.0, 1e-6], size=ls.m) * rng.uniform(0.5, 2.0, size=ls.m); sigma = 1e-6
    Pd = np.zeros((ls.n, ls.n)); Ad = np.zeros((ls.m, ls.n))
    B0 = rng.normal(size=(ls.n, ls.n)); Pv = np.zeros(ls.Pi.size)
    for j in range(ls.n):
        for k in range(ls.Pp[j], ls.Pp[j + 1]):
            Pv[k] = B0[min(ls.Pi[k], j), max(ls.Pi[k], j)]; Pd[ls.Pi[k], j] = Pv[k]
        for k in range(ls.Ap[j], ls.Ap[j + 1]):
            Ad[ls.Ai[k], j] = Av[k]
    npad, pos = info["npad"], a["pos"]
    M = np.eye(npad)
    M[np.ix_(pos, pos)] = Pd + sigma * np.eye(ls.n) + Ad.T @ (rho[:, None] * Ad)
    valA = np.where(a["A_src"] >= 0, Av[np.maximum(a["A_src"], 0)], 0.0); valAt = np.where(a["At_src"] >= 0, Av[np.maximum(a["At_src"], 0)], 0.0)
    valP = np.where(a["P_src"] >= 0, Pv[np.maximum(a["P_src"], 0)], 0.0)
    rho_pad = np.r_[rho, np.zeros(info["mpad"] - ls.m)]
    K = info["sing_k"]; ent = a["sing_ent"].reshape(K, npad); row = a["sing_row"].reshape(K, npad)
    d = np.where(a["perm"] >= 0, sigma + np.where(ent >= 0, rho_pad[np.maximum(row, 0)] * valAt[np.maximum(ent, 0)] ** 2, 0.0).sum(axis=0), 1.0)
    offs = np.array([[_off(r, c) for c in range(BS)] for r in range(BS)])
    lane = np.arange(WAVE); scale = np.abs(M).max(); worst = 0.0
    for p in range(info["t_parts"]):
        img = np.zeros(a["image"][p])
        sc = a["sc"][2 * a["sc_ptr"][p]:2 * a["sc_ptr"][p + 1]].reshape(-1, 2)
        packed = sc[:, 1].astype(np.int64) & 0xffffffff
        img[packed & 0xffff] = valA[sc[:, 0]] * np.sqrt(rho_pad[packed >> 16])
        tile = lambda s: img[s * BLK + offs]
        for b in range(a["blk0"][p], a["blk0"][p + 1]):
            S = np.zeros((BS, BS))
            for g in range(a["asm_ptr"][b], a["asm_ptr"][b + 1]):
                S += tile(a["ta"][g]) @ tile(a["tb"][g]).T
            for g in range(4):
                pi = a["asm_pidx"][b * BLK + g * WAVE + lane]
                S[(lane >> 4) + 4 * g, lane & 15] += np.where(pi >= 0, valP[np.maximum(pi, 0)], 0.0)
            J = a["blk_diag"][b]
            if J >= 0:
                S[np.arange(BS), np.arange(BS)] += d[J * BS:(J + 1) * BS]
            I, Jc = a["blkI"][b], a["blkJ"][b]
            worst = max(worst, np.abs(S - M[I * BS:(I + 1) * BS, Jc * BS:(Jc + 1) * BS]).max())
    assert worst <= 1e-13 * scale, (worst, scale)
    # ... and the blocks are all of M's lower triangle that is not zero
    cover = np.zeros((info["nb"], info["nb"]), bool); cover[a["blkI"], a["blkJ"]] = True
    nz = np.abs(M.reshape(info["nb"], BS, info["nb"], BS)).max(axis=(1, 3)) > 0
    assert not (np.tril(nz) & ~cover).any()
