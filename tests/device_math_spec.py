"""What tests/golden/make_device_math.py, tests/test_device_math.py and
tests/test_device_math_gpu.py share: the operations of tests/device_math_check (ids and case
widths as in device_math_check.h), how an output is made comparable, the error metric and the
case-file format. numpy only: nothing here imports mpmath.

Fixture layout (tests/golden/device_math.npz), per operation `op`:
  op/in       (n, win)  f64 inputs
  op/ref      (n, wc)   expected comparable output, the 50-digit value rounded to f64
  op/ref_lo   (n, wc)   only for the ulp-bounded operations: the 50-digit value minus op/ref
  op/alt      (n, wc)   NaN, or the other branch's value for a "+- ulps at a threshold" case
  op/cls      (n,)      class index of each case
  op/classes  (k,)      class names
  op/ecpu     (k,)      E_cpu: the plain-f64 baseline's largest error over the class
  op/bound    (k,)      what the device must meet: 16 * max(E_cpu, 2^-52), or the fixed rule

The comparable output of an operation is its raw output, except where a quaternion's sign or
Shepperd branch is not part of the contract: there the quaternion is replaced by R(q), Eigen's
toRotationMatrix polynomial (which also carries |q|).

Error of one case: over the operation's groups of output columns, the largest
|out - ref| / max(max |ref| over the group, the group's floor). A case with an `alt` row takes
the smaller of its two errors.
"""
from __future__ import annotations

import struct

import numpy as np

MAGIC = 0x31304B4843444D44
SENTINEL = -12345.0
EPS52 = 2.0 ** -52
MARGIN = 16.0

REL, EXACT, ULP = "rel", "exact", "ulp"


def quat_to_R(q):
    """Eigen toRotationMatrix on rows (x, y, z, w) -> (n, 9) row-major, in float64."""
    q = np.asarray(q, np.float64)
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.stack([1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz), tyz - twx,
                     txz - twy, tyz + twx, 1 - (txx + tyy)], axis=-1)


def _post_left_update(o):  # two (q, t) -> two (R, t)
    return np.concatenate([quat_to_R(o[:, 0:4]), o[:, 4:7], quat_to_R(o[:, 7:11]), o[:, 11:14]], 1)


def _post_sim3(o):  # (q, t, s) -> (R(q), t, s)
    return np.concatenate([quat_to_R(o[:, 0:4]), o[:, 4:8]], 1)


def _g(name, lo, hi, kind=REL, floor=0.0):
    return (name, slice(lo, hi), kind, floor)


# name -> id, doubles in, doubles out, group list over the comparable columns, post transform
OPS = {
    "rcp_nr": dict(id=1, win=1, wout=1, groups=[_g("y", 0, 1, ULP)]),
    "rsq_nr": dict(id=2, win=1, wout=1, groups=[_g("y", 0, 1, ULP)]),
    "huber": dict(id=3, win=2, wout=4, groups=[_g("rho0", 0, 1, ULP), _g("rho0_sel", 1, 2, ULP),
                                                _g("rho01_r0", 2, 3, ULP), _g("rho01_r1", 3, 4, ULP)]),
    "ldlt_solve6": dict(id=4, win=28, wout=7, groups=[_g("ok", 0, 1, EXACT), _g("x", 1, 7)]),
    "left_update": dict(id=5, win=13, wout=14, post=_post_left_update,
                        groups=[_g("pose_R", 0, 9, REL, 1.0), _g("pose_t", 9, 12, REL, 1.0),
                                _g("se3_R", 12, 21, REL, 1.0), _g("se3_t", 21, 24, REL, 1.0)]),
    "quat_from_R": dict(id=6, win=9, wout=4, groups=[_g("q", 0, 4, REL, 1.0)]),
    "normalize_rotation": dict(id=7, win=4, wout=4, groups=[_g("q", 0, 4, REL, 1.0)]),
    "quat_rotate": dict(id=8, win=7, wout=3, groups=[_g("v", 0, 3)]),
    "quat_to_R": dict(id=9, win=4, wout=9, groups=[_g("R", 0, 9, REL, 1.0)]),
    "sim3_exp": dict(id=10, win=7, wout=8, post=_post_sim3,
                     groups=[_g("R", 0, 9, REL, 1.0), _g("t", 9, 12), _g("s", 12, 13)]),
    "sim3_log": dict(id=11, win=8, wout=7,
                     groups=[_g("omega", 0, 3), _g("upsilon", 3, 6), _g("sigma", 6, 7, REL, 1e-5)]),
    "sim3_mul": dict(id=12, win=16, wout=8, groups=[_g("q", 0, 4), _g("t", 4, 7), _g("s", 7, 8)]),
    "sim3_inverse": dict(id=13, win=8, wout=8, groups=[_g("q", 0, 4), _g("t", 4, 7), _g("s", 7, 8)]),
    "sim3_affine": dict(id=14, win=8, wout=12, groups=[_g("sR", 0, 9), _g("t", 9, 12)]),
    "lu3_solve": dict(id=15, win=12, wout=3, groups=[_g("x", 0, 3)]),
    "tri_rc": dict(id=16, win=1, wout=2, groups=[_g("rc", 0, 2, EXACT)]),
    "diag_ldlt": dict(id=17, win=27, wout=34, groups=[_g("good", 0, 1, EXACT), _g("A", 1, 22),
                                                       _g("y", 22, 28), _g("rdg", 28, 34)]),
    "panel_row": dict(id=18, win=34, wout=13, groups=[_g("v", 0, 6), _g("l", 6, 12), _g("r", 12, 13)]),
    "block_back6": dict(id=19, win=21, wout=6, groups=[_g("x", 0, 6)]),
    "factor_diag_block": dict(id=20, win=90, wout=130,
                              groups=[_g("good", 0, 1, EXACT), _g("Lp", 1, 79), _g("rhs", 79, 91),
                                      _g("dg_head", 91, 97, EXACT), _g("dg", 97, 103),
                                      _g("idg_head", 103, 109, EXACT), _g("idg", 109, 115),
                                      _g("L15", 115, 130)]),
    "block_solve": dict(id=21, win=190, wout=19, groups=[_g("ok", 0, 1, EXACT), _g("x", 1, 19)]),
    "eval_edge": dict(id=22, win=24, wout=9,
                      groups=[_g("chi2", 0, 1, REL, 1.0), _g("e", 1, 4, REL, 1.0), _g("xy", 4, 6, REL, 1.0),
                              _g("iz", 6, 7), _g("stereo_info", 7, 9, EXACT)]),
    "ldlt_solve7": dict(id=30, win=36, wout=8, groups=[_g("ok", 0, 1, EXACT), _g("x", 1, 8)]),
    "huber_sim3": dict(id=31, win=2, wout=2, groups=[_g("r0", 0, 1, ULP), _g("r1", 1, 2, ULP)]),
    "eg_edge_error": dict(id=40, win=24, wout=8, groups=[_g("e", 0, 7, REL, 1.0), _g("chi2", 7, 8, REL, 1.0)]),
    "eg_oplus_axis": dict(id=41, win=11, wout=8, post=_post_sim3,
                          groups=[_g("R", 0, 9, REL, 1.0), _g("t", 9, 12, REL, 1.0), _g("s", 12, 13)]),
}

# The operations one child process of the GPU test runs together.
GROUPS = {
    "recip_huber": ["rcp_nr", "rsq_nr", "huber", "huber_sim3"],
    "ldlt": ["ldlt_solve6", "ldlt_solve7"],
    "se3": ["left_update", "quat_from_R", "normalize_rotation", "quat_rotate", "quat_to_R"],
    "sim3": ["sim3_exp", "sim3_log", "sim3_mul", "sim3_inverse", "sim3_affine", "lu3_solve"],
    "eg": ["eg_edge_error", "eg_oplus_axis"],
    "pose_edge": ["eval_edge"],
    "ba_ldlt": ["tri_rc", "diag_ldlt", "panel_row", "block_back6", "factor_diag_block",
                "block_solve"],
}

# Classes every operation must carry, with their minimum case counts (the fixture test).
MIN_CASES = {
    "rcp_nr": {"log_uniform": 64, "pow2": 64, "near_one": 32, "pivots": 64},
    "rsq_nr": {"log_uniform": 64, "pow2": 64, "near_one": 32, "pivots": 64},
    "huber": {"mono": 5, "stereo": 5},
    "huber_sim3": {"mono": 5, "stereo": 5},
    "ldlt_solve6": {"spd_well": 64, "spd_ill": 64, "zero_rowcol": 12, "indefinite": 6},
    "ldlt_solve7": {"spd_well": 64, "spd_ill": 64, "zero_rowcol": 14, "fix_scale": 8,
                    "indefinite": 7},
    "left_update": {"theta_zero": 8, "theta_1e-12": 8, "thr_t2_1e-10": 6, "taylor": 64,
                    "thr_t2_1e-4": 6, "generic": 64, "trace_sign": 16, "near_pi": 64,
                    "past_pi": 64},
    "quat_from_R": {"generic": 64, "near_pi": 64, "ties": 6},
    "normalize_rotation": {"generic": 64},
    "quat_rotate": {"generic": 64},
    "quat_to_R": {"generic": 64},
    "sim3_exp": {"small_theta_small_sigma": 16, "small_theta": 16, "small_sigma": 16,
                 "thr_theta": 6, "thr_sigma": 6, "generic": 64, "past_pi": 64},
    "sim3_log": {"generic": 64, "norm_off": 64, "thr_d": 6, "thr_sigma": 6, "pi_1e-2": 16,
                 "pi_1e-4": 16, "small_theta_small_sigma": 16, "small_sigma": 16, "small_theta": 16},
    "sim3_mul": {"generic": 64},
    "sim3_inverse": {"generic": 64},
    "sim3_affine": {"generic": 64},
    "lu3_solve": {"pivot_orders": 48, "near_tied": 16},
    "tri_rc": {"all": 171},
    "diag_ldlt": {"spd": 64, "zero_pivot": 6, "negative_pivot": 6},
    "panel_row": {"generic": 64},
    "block_back6": {"generic": 64},
    "factor_diag_block": {"spd": 64},
    "block_solve": {"K1_well": 16, "K2_well": 16, "K3_well": 16, "K1_ill": 16, "K2_ill": 16,
                    "K3_ill": 16},
    "eval_edge": {"mono": 64, "stereo": 64, "octave_clamps": 16, "quotient": 256},
    "eg_edge_error": {"consistent": 32, "random": 64, "half_turn": 16},
    "eg_oplus_axis": {"fix_scale_off": 42, "fix_scale_on": 42},
}

# Classes whose E_cpu the generator caps at 1e-13 (well-conditioned: issue section 4).
CAPPED = {
    "sim3_exp": ["generic", "past_pi"], "sim3_mul": ["generic"], "sim3_inverse": ["generic"],
    "sim3_affine": ["generic"], "ldlt_solve6": ["spd_well"], "ldlt_solve7": ["spd_well"],
    "block_solve": ["K1_well", "K2_well", "K3_well"],
}
CAP = 1e-13
ALT_SHARE = 0.05


def comparable(op: str, raw: np.ndarray) -> np.ndarray:
    post = OPS[op].get("post")
    return post(raw) if post else raw


def case_errors(op: str, out: np.ndarray, ref: np.ndarray, ref_lo=None, alt=None, only=None):
    """(n,) error of each case of comparable `out` against the fixture rows; ULP groups count in
    ulps of ref, EXACT groups give 0 or inf, REL groups are relative to the group's scale.
    `only`: the names of the groups to look at (default: all)."""
    def one(r, lo):
        err = np.zeros(len(out))
        for name, sl, kind, floor in OPS[op]["groups"]:
            if only is not None and name not in only:
                continue
            o, rr = out[:, sl], r[:, sl]
            if kind == EXACT:
                e = np.where((o == rr).all(1), 0.0, np.inf)
            elif kind == ULP:
                d = (o - rr) - (lo[:, sl] if lo is not None else 0.0)
                e = (np.abs(d) / np.spacing(np.abs(rr))).max(1)
            else:
                scale = np.maximum(np.abs(rr).max(1), floor)
                scale = np.where(scale > 0, scale, 1.0)
                e = np.abs(o - rr).max(1) / scale
            e = np.where(np.isfinite(o).all(1), e, np.inf)
            err = np.maximum(err, e)
        return err

    err = one(ref, ref_lo)
    if alt is not None:
        has = ~np.isnan(alt).any(1)
        if has.any():
            e2 = one(np.where(has[:, None], alt, ref), None)
            err = np.where(has, np.minimum(err, e2), err)
    return err


def write_case_file(path: str, ops, fixture) -> None:
    with open(path, "wb") as f:
        f.write(struct.pack("<QQ", MAGIC, len(ops)))
        for op in ops:
            a = np.ascontiguousarray(fixture[op + "/in"], np.float64)
            s = OPS[op]
            assert a.ndim == 2 and a.shape[1] == s["win"], op
            f.write(struct.pack("<QQQQ", s["id"], a.shape[0], s["win"], s["wout"]))
            f.write(a.tobytes())


def read_result_file(path: str, ops, fixture) -> dict:
    """Raw outputs by operation; every header field is checked against what was sent."""
    with open(path, "rb") as f:
        buf = f.read()
    magic, nrec = struct.unpack_from("<QQ", buf, 0)
    assert magic == MAGIC and nrec == len(ops), "result header"
    at, res = 16, {}
    for op in ops:
        s, n = OPS[op], fixture[op + "/in"].shape[0]
        assert struct.unpack_from("<QQQQ", buf, at) == (s["id"], n, s["win"], s["wout"]), op
        at += 32
        res[op] = np.frombuffer(buf, np.float64, n * s["wout"], at).reshape(n, s["wout"]).copy()
        at += 8 * n * s["wout"]
    assert at == len(buf), "result length"
    return res


# Where the expected value is an exact zero (a zero pivot's component, its reciprocal) or the
# sentinel (a failed solve leaves x alone), the output must equal it bit for bit.
EXACT_WHERE_REF = {"ldlt_solve6": (slice(1, 7), (0.0, SENTINEL)),
                   "ldlt_solve7": (slice(1, 8), (0.0, SENTINEL)),
                   "diag_ldlt": (slice(28, 34), (0.0,))}


def oracle_baseline(op: str, inp: np.ndarray):
    """The oracle's exported float64 primitives (oracle/sim3_oracle.h, se3_oracle.h through
    tests/oracle_lib.py) on the fixture inputs of `op`, as comparable rows; None for an
    operation the oracle exports nothing for."""
    import oracle_lib as O

    def rows(f):
        return np.array([f(r) for r in np.asarray(inp, np.float64)])

    def left_update(r):  # oc_se3_exp gives R, t of exp(u); composed with T in float64
        R, t = O.se3_exp(r[:6].copy())
        RT = quat_to_R(r[None, 6:10])[0].reshape(3, 3)
        b = np.concatenate([(R @ RT).ravel(), t + R @ r[10:13]])
        return np.concatenate([b, b])

    def eg_error(r):
        e = O.sim3_log(O.sim3_mul(O.sim3_mul(r[0:8].copy(), r[8:16].copy()),
                                  O.sim3_inverse(r[16:24].copy())))
        return np.concatenate([e, [float((e * e).sum())]])

    def eg_oplus(r):
        u = np.zeros(7)
        u[int(r[8])] = r[9]
        if r[10]:
            u[6] = 0.0
        return _post_sim3(O.sim3_mul(O.sim3_exp(u), r[:8].copy())[None])[0]

    f = {"left_update": left_update,
         "sim3_exp": lambda r: _post_sim3(O.sim3_exp(r.copy())[None])[0],
         "sim3_log": lambda r: O.sim3_log(r.copy()),
         "sim3_mul": lambda r: O.sim3_mul(r[:8].copy(), r[8:].copy()),
         "sim3_inverse": lambda r: O.sim3_inverse(r.copy()),
         "eg_edge_error": eg_error, "eg_oplus_axis": eg_oplus}.get(op)
    return rows(f) if f else None
