"""Placement relocation (csrc/krcn_place.hip): the probe of a plan build and the
search over the first Lanczos calls move every hot buffer of a handle (both
plans' tables, u, tn, W, td, pa, pb, pz, pq) to fresh allocations, and
include/krcn.h promises that no result changes by it.

krcn_csr_set_placement_keep(k - 1) makes every run keep the last copy, so the
buffers really move each time.  Every comparison has two legs, neither of them
the code under test:
  leg 1  bitwise against a handle of the same matrix, policy and inputs with
         set_placement_trials(0) (the header's contract);
  leg 2  against the reference the existing test of that call uses, at that
         test's tolerance: the f1 goldens at 1e-13 for matvec, rmatvec and hvp
         (test_gpu_hvp.py), scipy + logistic_ref.py at 1e-13 for the gradient
         and the loss, the f2 goldens at 1e-11 for Lanczos (test_gpu_lanczos.py;
         1e-9 on the long-row operator, test_gpu_tiling.py; 1e-10 against the
         CGS2 oracle with reorth), a dense solve at 1e-8 for cg_solve
         (test_gpu_methods.py), the oracle's Krylov-CRN step at 1e-10 for
         crn_step (test_gpu_crn.py), fp32 handles at 1e-5 and the leading four
         Lanczos coefficients at 1e-4 (test_gpu_window.py).

What each group would catch (argued from the code, never run against it):
  a. lazy build as the first compute call: an entry point that reads u / tn /
     td before plans_for_compute hands the kernels a freed buffer (keep > 0);
     a gradient whose residual is queued before the build loses it to the
     probe's zero-fill of tn (any keep, keep = 0 included);
  b. every plan family: PlaceSet::apply forgetting an aliased ptr / idx / val
     (sliced plans), re-pointing one that is the handle's own array (unsliced
     wave), a slot missing from hot_slots, or a copy shorter than its table
     entry changes a result or a plan readout;
  c. the Lanczos-call search: lzp_begin applying a copy after a pointer was
     read, lzp_done keeping a freed candidate, a candidate copied before the
     previous call's work on its stream, the timed-call bookkeeping;
  d. an interrupted search: lzp_abort freeing the applied placement, or not
     freeing the others before a rebuild replaces the tables' fields.
"""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import krcn
import krcn_oracle as O
import logistic_ref as R
from conftest import golden_csr, load_golden, rel_err
from krcn import _lib
from test_gpu_lanczos import D_PAD, EARLY_PLANS, FUSED_PLANS, pad_cols
from test_gpu_tiling import long_row_matrix

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64, F32 = torch.float64, torch.float32
WAVE, WINDOW, JAG, DENSE = krcn.KRCN_FORMAT_WAVE, krcn.KRCN_FORMAT_WINDOW, krcn.KRCN_FORMAT_JAG, 5
WIN_JAG = EARLY_PLANS["early_jag"]   # news20's plans: window-slices pass 1, jagged pass 2
L2 = 0.01
OPS = ["matvec", "rmatvec", "hvp", "hvp_l2", "gradient", "gradient_l2", "loss_values", "cg_solve", "crn_step",
       "lanczos", "hvp_block"]


def h(x):
    return x.cpu().numpy()


def pad(v, d):
    return np.concatenate([v, np.zeros(d - len(v))])


def f32_round(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


def lz_info(info):
    return np.array([info.m_eff, info.breakdown, info.j_break, info.hvps, info.beta_last, info.gnorm])


class Problem:
    """A matrix, a plan policy, a dtype and host inputs; the host references of
    every op (leg 2) and the outputs of a handle without the placement search
    (leg 1), each computed once and shared read-only.

    A is the matrix whose values the handle holds (values="f32": rounded to
    fp32); the host inputs of an fp32 handle are fp32-representable, so its
    references are those of what the device is given."""

    def __init__(self, A, policy, x, b01, v, dtype=F64, V3=None, values=0, A_handle=None):
        self.A, self.policy, self.dtype, self.values = sp.csr_matrix(A), dict(policy), dtype, values
        self.A_handle = self.A if A_handle is None else A_handle
        self.n, self.d = self.A.shape
        cast = f32_round if dtype == F32 else np.asarray
        if dtype == F32:
            self.A = sp.csr_matrix((f32_round(self.A.data), self.A.indices, self.A.indptr), shape=self.A.shape)
        self.x, self.b01, self.v = cast(x), np.asarray(b01, dtype=np.float64), cast(v)
        self.Ax = cast(self.A @ self.x)
        self.u = cast(R.np_expit(self.Ax) - self.b01)
        self.w = cast(O.hessian_weights(self.A, self.x))
        self.g = cast(self.A.T @ self.u / self.n)
        self.V3 = cast(np.stack([self.v, np.roll(self.v, 1), self.v[::-1]], axis=1) if V3 is None else V3)
        self.value = float(np.mean((1 - self.b01) * self.Ax - R.np_logsig(self.Ax)))
        self.tol = 1e-13 if dtype == F64 else 1e-5
        self.lz_tol = 1e-11
        self.lz_ref = {}      # (m, reorth, l2) -> (alphas, betas, V or None), golden overrides
        self.ref = {}         # op -> host reference arrays, golden overrides
        self._base = {}
        self._base_handle = None

    # -- device side ---------------------------------------------------------
    def t(self, a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, self.dtype)

    def handle(self, trials, keep=-1, **kw):
        """A fresh handle: its policy set, no plan built."""
        X = krcn.DeviceCSR(self.A_handle, dtype=self.dtype, values=self.values, **dict(self.policy, **kw))
        X.set_placement_trials(trials)
        X.set_placement_keep(keep)
        return X

    def lanczos(self, X, m, reorth=False, l2=0.0, V=None):
        V = torch.zeros((m, self.d), dtype=self.dtype, device=DEV) if V is None else V   # (whole V is compared)
        V, al, be, info = X.lanczos(self.t(self.w), self.t(self.g), m, reorth=reorth, l2=l2, V=V)
        return [al, be, lz_info(info), h(V)]

    def run(self, X, op):
        """The outputs of one op as numpy arrays."""
        t = self.t
        if op == "matvec":
            return [h(X.matvec(t(self.x)))]
        if op == "rmatvec":
            return [h(X.rmatvec(t(self.u)))]
        if op in ("hvp", "hvp_l2"):
            return [h(X.hvp(t(self.w), t(self.v), l2=L2 if op == "hvp_l2" else 0.0))]
        if op == "gradient":
            return [h(X.gradient(t(self.Ax), t(self.b01)))]
        if op == "gradient_l2":
            return [h(X.gradient(t(self.Ax), t(self.b01), t(self.x), l2=L2))]
        if op == "loss_values":
            return [np.array(X.loss_values([t(self.x), t(0.1 * self.v)], t(self.b01)))]
        if op == "cg_solve":
            sol, ci = X.cg_solve(t(self.w), t(self.v), shift=0.05, rtol=1e-10)
            return [h(sol), np.array([ci.converged, ci.info, ci.iterations, ci.residual_norm])]
        if op == "crn_step":
            V = torch.zeros((10, self.d), dtype=self.dtype, device=DEV)
            x_new, Ax_new, al, be, ci = X.crn_step(t(self.x), t(self.b01), self.value, 10, 1e-3, Ax=t(self.Ax), V=V)
            return [h(x_new), h(Ax_new), al, be, h(V), lz_info(ci.lanczos),
                    np.array([ci.accepted, ci.trials, ci.solver_it, ci.solver_status, ci.reg_coef, ci.lam,
                              ci.model_decrease, ci.value_new, ci.dx_norm])]
        if op == "lanczos":
            return self.lanczos(X, 10)
        if op == "hvp_block":
            return [h(X.hvp_block(t(self.w), t(self.V3)))]
        raise KeyError(op)

    def base(self, op):
        """Leg 1's other side: the op on a handle with the placement code off."""
        if op not in self._base:
            if self._base_handle is None:
                self._base_handle = self.handle(0)
            self._base[op] = self.run(self._base_handle, op)
            assert self._base_handle.placement_info()["probed"] == 0
        return self._base[op]

    # -- host side -----------------------------------------------------------
    def lanczos_reference(self, m, reorth=False, l2=0.0):
        key = (m, bool(reorth), l2)
        if key not in self.lz_ref:
            fn = O.lanczos_cgs2 if reorth else O.lanczos
            V, al, be, _ = fn(lambda q: O.hvp_from_weights(self.A, self.w, q, l2), self.g, m)
            self.lz_ref[key] = (al, be, V)
        return self.lz_ref[key]

    def reference(self, op):
        if op in self.ref:
            return self.ref[op]
        A, n = self.A, self.n
        if op == "matvec":
            r = [A @ self.x]
        elif op == "rmatvec":
            r = [A.T @ self.u / n]
        elif op in ("hvp", "hvp_l2"):
            r = [O.hvp_from_weights(A, self.w, self.v, L2 if op == "hvp_l2" else 0.0)]
        elif op in ("gradient", "gradient_l2"):
            r = [A.T @ (R.np_expit(self.Ax) - self.b01) / n + (L2 * self.x if op == "gradient_l2" else 0.0)]
        elif op == "loss_values":
            r = [np.array([np.mean((1 - self.b01) * (A @ z) - R.np_logsig(A @ z)) for z in (self.x, 0.1 * self.v)])]
        elif op == "cg_solve":
            live = np.flatnonzero(np.diff(A.tocsc().indptr))   # empty columns: H is zero there, x = b / shift
            Al = A[:, live]
            H = (Al.T.multiply(self.w) @ Al / n).toarray() + 0.05 * np.eye(len(live))
            sol = self.v / 0.05
            sol[live] = np.linalg.solve(H, self.v[live])
            r = [sol]
        elif op == "crn_step":
            live = slice(0, int(A.indices.max()) + 1)          # (the oracle's dense T solve does not need the padding)
            tr = O.krylov_crn(A[:, live], 2 * self.b01 - 1, self.x[live], m=10, reg_coef=1e-3, it_max=1)
            x_new = self.x.copy()
            x_new[live] = tr["xs"][-1]
            r = [x_new, float(tr["value"][-1]), float(tr["reg_coef"][-1])]
        elif op == "hvp_block":
            r = [np.stack([O.hvp_from_weights(A, self.w, self.V3[:, j]) for j in range(self.V3.shape[1])], axis=1)]
        else:
            raise KeyError(op)
        self.ref[op] = r
        return r

    def check_lanczos(self, out, m, reorth=False, l2=0.0):
        al, be, info, V = out
        al_r, be_r, V_r = self.lanczos_reference(m, reorth, l2)
        assert info[0] == len(al_r) == m and not info[1]
        if self.dtype == F32:
            assert rel_err(al[:4], al_r[:4]) < 1e-4 and rel_err(be[:4], be_r[:4]) < 1e-4
            return
        tol = 1e-10 if reorth else self.lz_tol
        assert rel_err(al, al_r) < tol
        assert rel_err(be, be_r) < tol
        if V_r is not None and tol <= 1e-10:
            d0 = V_r.shape[0]
            assert np.abs(V[:m, :d0].T - V_r).max() < 1e-6
            assert np.all(V[:m, d0:] == 0)

    def check(self, op, out):
        """Leg 2."""
        if op == "lanczos":
            return self.check_lanczos(out, 10)
        ref = self.reference(op)
        if op == "cg_solve":
            assert out[1][0] == 1 and out[1][1] == 0
            assert rel_err(out[0], ref[0]) < (1e-8 if self.dtype == F64 else 1e-3)
        elif op == "crn_step":
            x_new, Ax_new, al, be, V, li, ci = out
            assert ci[0] == 1 and ci[4] == ref[2]
            assert rel_err(x_new, ref[0]) < 1e-10
            assert rel_err(Ax_new, self.A @ ref[0]) < 1e-10
            assert abs(ci[7] - ref[1]) <= 1e-10 * abs(ref[1])
            self.check_lanczos([al, be, li, V], 10)
        elif op == "loss_values":
            assert np.all(np.abs(out[0] - ref[0]) <= self.tol * np.abs(ref[0]))
        else:
            assert rel_err(out[0], ref[0]) < self.tol

    def check_both(self, X, op, what=""):
        out = self.run(X, op)
        for k, (a, b) in enumerate(zip(out, self.base(op))):
            np.testing.assert_array_equal(a, b, err_msg=f"{what} {op} output {k}: differs from the handle "
                                                        "without the placement search")
        self.check(op, out)
        return out


# ------------------------------------------------------------------ problems
_PROBLEMS = {}


def f1_problem(policy, padded, dtype=F64, values=0):
    """f1's operator at x0 (optionally padded to D_PAD empty columns, as test_gpu_lanczos.py pads it),
    with the goldens as the references wherever the handle holds f1's own values."""
    f1, f2 = load_golden("f1_hvp.npz"), load_golden("f2_lanczos.npz")
    A0 = golden_csr(f1)
    d0 = A0.shape[1]
    d = D_PAD if padded else d0
    A = pad_cols(A0, d)
    Ah = A
    if values:   # the fp64 matrix the narrowed plans hold
        A = sp.csr_matrix((f32_round(A.data), A.indices, A.indptr), shape=A.shape)
    P = Problem(A, policy, pad(f1["x0"], d), O.labels01(f1["b"]), pad(f1["v0"], d), dtype=dtype,
                V3=np.stack([pad(f1[f"v{k}"], d) for k in range(3)], axis=1), values=values, A_handle=Ah)
    if dtype == F64 and not values:
        # the host inputs are the goldens' to rounding, so the goldens are the references
        assert rel_err(P.Ax, f1["Ax0"]) < 1e-14 and rel_err(P.g[:d0], f2["g"]) < 1e-14
        P.ref.update(matvec=[f1["Ax0"]], rmatvec=[pad(f1["grad0"], d)], hvp=[pad(f1["hvp0_0"], d)],
                     hvp_l2=[pad(f1["hvp0_0_l2"], d)],
                     hvp_block=[np.stack([pad(f1[f"hvp0_{k}"], d) for k in range(3)], axis=1)])
        P.lz_ref[(10, False, 0.0)] = (f2["alphas_m10"], f2["betas_m10"], f2["V_m10"])
    return P


def long_rows_problem():
    A, b = long_row_matrix()
    P = Problem(A, dict(fmt=JAG), np.random.default_rng(1).uniform(-0.2, 0.2, size=A.shape[1]), O.labels01(b),
                np.random.default_rng(2).standard_normal(A.shape[1]))
    P.lz_tol = 1e-9   # test_gpu_tiling.py: this skewed operator amplifies rounding
    return P


def dense_problem():
    f8 = load_golden("f8_dense.npz")
    P = Problem(golden_csr(f8), dict(fmt=DENSE), f8["x"], f8["b01"], f8["v0"])
    P.ref.update(matvec=[f8["Ax_l2_0"]], hvp=[f8["hvp0_l2_0"]], hvp_l2=[f8["hvp0_l2_1"]], gradient=[f8["grad_l2_0"]])
    assert rel_err(P.g, f8["g"]) < 1e-14
    P.lz_ref[(10, False, 0.0)] = (f8["alphas_m10"], f8["betas_m10"], f8["V_m10"])
    return P


MAKERS = {
    "win_jag": lambda: f1_problem(WIN_JAG, True),
    "win_jag_f32": lambda: f1_problem(WIN_JAG, True, dtype=F32),
    "win_jag_values32": lambda: f1_problem(WIN_JAG, True, values="f32"),
    "win_acc": lambda: f1_problem(EARLY_PLANS["early_win"], True),
    "early_sorted": lambda: f1_problem(EARLY_PLANS["early_sorted"], True),
    "fused_win": lambda: f1_problem(FUSED_PLANS["fused_win"], True),
    "sorted8": lambda: f1_problem(FUSED_PLANS["sorted"], False),
    "sorted8_f32": lambda: f1_problem(FUSED_PLANS["sorted"], False, dtype=F32),
    "two_launch": lambda: f1_problem(FUSED_PLANS["two_launch"], False),
    "one_piece": lambda: f1_problem(FUSED_PLANS["small"], False),
    "wave": lambda: f1_problem(dict(fmt=WAVE, slicing=1), False),
    "jag_long": long_rows_problem,
    "dense": dense_problem,
}
EXPECT_FORMAT = {
    "win_jag": ("window-slices", "jagged"),
    "win_jag_f32": ("window-accum", "jagged"),   # (fp32 windows hold twice the entries: too few slices to split)
    "win_jag_values32": ("window-slices", "jagged"), "win_acc": ("window-slices", "window-accum"),
    "early_sorted": ("sorted", "jagged"), "fused_win": ("window-slices", "sorted"), "sorted8": ("sorted", "sorted"),
    "sorted8_f32": ("sorted", "sorted"), "two_launch": ("sorted", "jagged"), "one_piece": ("window-accum", "window-accum"),
    "wave": ("wave", "wave"), "jag_long": ("jagged", "jagged"), "dense": ("dense", "dense"),
}
# FUSED_PLANS / EARLY_PLANS kinds of test_gpu_lanczos.py -> the problem on those plans and the step it must take
SEARCH = {"sorted": ("sorted8", "fused-sorted"), "small": ("one_piece", "fused-small-xt"),
          "two_launch": ("two_launch", "two-launch"), "fused_win": ("fused_win", "fused-window"),
          "early_jag": ("win_jag", "early"), "early_win": ("win_acc", "early"), "early_sorted": ("early_sorted", "early"),
          "wave": ("wave", "generic")}
assert set(SEARCH) == set(FUSED_PLANS) | set(EARLY_PLANS) | {"wave"}


def problem(name):
    if name not in _PROBLEMS:
        _PROBLEMS[name] = MAKERS[name]()
    return _PROBLEMS[name]


def expect_format(X, name):
    fmt = X.plan_format()
    assert (fmt["pass1"], fmt["pass2"]) == EXPECT_FORMAT[name]


def assert_probe(X, k, keep):
    info = X.placement_info()
    assert info["probed"] == k and info["kept"] == keep and info["policy"] == k and info["keep"] == keep
    assert len(info["us"]) == k and all(u > 0 for u in info["us"])
    return info


def first_call(P, name, op, k, keep, **kw):
    """The op as the first compute call of a fresh handle (its plan build, probe and relocation
    run inside it), then once more; nothing before it builds the plans."""
    X = P.handle(k, keep, **kw)
    P.check_both(X, op, "first call:")
    P.check_both(X, op, "second call:")
    assert_probe(X, k, keep)
    expect_format(X, name)
    return X


# ------------------------------------------------- a. lazy build, first call
@pytest.mark.parametrize("k,keep", [(2, 0), (2, 1), (4, 0), (4, 3)])
@pytest.mark.parametrize("op", OPS)
def test_first_call_builds_probes_and_relocates(op, k, keep):
    first_call(problem("win_jag"), "win_jag", op, k, keep)


@pytest.mark.parametrize("k,keep", [(2, 0), (2, 1), (4, 0), (4, 3)])
@pytest.mark.parametrize("op", ["hvp", "hvp_l2", "gradient", "gradient_l2"])
def test_first_call_sorted_slices(op, k, keep):
    first_call(problem("sorted8"), "sorted8", op, k, keep)


@pytest.mark.parametrize("mode", [_lib.KRCN_SHARD_ROWS, _lib.KRCN_SHARD_COLS])
@pytest.mark.parametrize("op", ["hvp", "hvp_l2", "gradient", "gradient_l2"])
def test_first_call_shard_modes_without_communicator(op, mode):
    """A ROWS handle's X^T pass goes through td (xt_pass), a COLS handle's X pass through u; without a
    communicator every all-reduce is the identity, so f1's goldens hold."""
    P = problem("sorted8")
    X = P.handle(3, 2, shard_mode=mode)
    B = P.handle(0, shard_mode=mode)
    for call in range(2):
        out, base = P.run(X, op), P.run(B, op)
        np.testing.assert_array_equal(out[0], base[0])
        P.check(op, out)
    assert_probe(X, 3, 2)
    assert B.placement_info()["probed"] == 0


@pytest.mark.parametrize("name", ["win_jag_f32", "sorted8_f32"])
@pytest.mark.parametrize("op", ["hvp", "gradient_l2", "lanczos"])
def test_first_call_fp32_handle(op, name):
    first_call(problem(name), name, op, 2, 1)


@pytest.mark.parametrize("op", ["hvp", "gradient"])
def test_first_call_most_placements(op):
    first_call(problem("win_jag"), "win_jag", op, 8, 7)   # kPlaceMax


def test_rebuild_mid_life_first_call_is_gradient():
    """A handle that has computed, then a policy call: the rebuild (with its probe and relocation)
    runs inside the gradient that follows, after the residual's scratch has been in use."""
    P, Q = problem("sorted8"), problem("wave")
    X = first_call(P, "sorted8", "hvp", 3, 2)
    P.check_both(X, "lanczos")
    X.set_slicing(1)
    X.set_format(WAVE)
    Q.check_both(X, "gradient_l2", "after set_format:")
    assert_probe(X, 3, 2)
    expect_format(X, "wave")
    for op in ("gradient", "hvp", "matvec", "lanczos"):
        Q.check_both(X, op, "after set_format:")
    X.set_placement_keep(0)   # a change of the override alone rebuilds too
    Q.check_both(X, "gradient", "after set_placement_keep:")
    assert_probe(X, 3, 0)


def test_keep_is_clamped_and_range_checked_on_a_live_handle():
    """keep = 7 with three placements keeps the last one in both searches; a value outside -1..7 is
    refused and leaves the override, the plans and the kept placement as they were."""
    P = problem("sorted8")
    X = P.handle(3, 7)
    P.check_both(X, "gradient", "first call:")
    info = X.placement_info()
    assert info["probed"] == 3 and info["kept"] == 2 and info["keep"] == 7
    for bad in (-2, 8):
        with pytest.raises(krcn.KrcnError, match="0..7"):
            X.set_placement_keep(bad)
    assert X.placement_info()["keep"] == 7
    for call in range(4):   # warm, then placements 0, 1, 2
        P.check_both(X, "lanczos")
    lz = X.placement_info()["lanczos"]
    assert lz["timed"] == 3 and lz["stage"] == -1 and lz["kept"] == 2   # (no rebuild in between: the search finished)
    P.check_both(X, "hvp")


# ------------------------------------------- b. every plan family relocates
@pytest.mark.parametrize("name", ["wave", "sorted8", "one_piece", "win_acc", "win_jag", "jag_long", "dense",
                                  "win_jag_values32"])
def test_every_family_relocates(name):
    P = problem(name)
    X, B = P.handle(3, 2), P.handle(0)   # (a fresh pair: owned_bytes counts the workspaces of the calls made)
    for op in ("matvec", "rmatvec", "hvp", "hvp_l2", "gradient", "gradient_l2", "lanczos"):
        P.check_both(X, op, name)
        P.run(B, op)
    assert_probe(X, 3, 2)
    expect_format(X, name)
    assert B.placement_info()["probed"] == 0
    assert X.plan_format() == B.plan_format()
    assert X.plan_info() == B.plan_info()
    assert X.plan_value_bytes() == B.plan_value_bytes()
    assert X.plan_value_bytes()["pass1"] == (4 if name == "win_jag_values32" else 8)
    assert X.lanczos_step() == B.lanczos_step() and X.lanczos_step(reorth=True) == B.lanczos_step(reorth=True)
    assert X.owned_bytes() == B.owned_bytes()
    if name == "wave":      # unsliced: ptr / idx / val are the handle's own arrays, which never move
        assert X.plan_info()["pass1"][0] == 1 and X.plan_info()["pass2"][0] == 1
    if name == "sorted8":   # sliced: they are the plan's owned copies, which do
        assert X.plan_info()["pass1"][0] == -8


# -------------------------------------------- c. the search over Lanczos calls
def search_sequence(P, X, l2=0.0):
    """The calls of one search (k = 3): which are timed is in the comments."""
    out = []
    lz = lambda m, **kw: out.append((("lanczos", m, kw.get("reorth", False)), P.lanczos(X, m, l2=l2, **kw)))  # noqa: E731
    lz(10)                   # 1. the warm call
    lz(5)                    # 2. ineligible: m < 8
    lz(10)                   # 3. timed: placement 0
    out.append((("hvp",), P.run(X, "hvp")))
    out.append((("gradient",), P.run(X, "gradient")))
    lz(12)                   # 5. another m: not timed
    X.reserve(12, reorth=True)
    lz(10, reorth=True)      # 6. timed: placement 1, a fresh copy
    lz(10)                   # 7. timed: placement 2; the search ends and keeps one
    lz(10)                   # 8. on the kept placement, the others freed
    lz(10)
    return out


def check_search(P, X, keep, step, l2=0.0):
    B = P.handle(0)
    got, base = search_sequence(P, X, l2), search_sequence(P, B, l2)
    assert X.lanczos_step() == B.lanczos_step() and step in (None, X.lanczos_step())
    for (what, a), (_, b) in zip(got, base):
        for k, (ai, bi) in enumerate(zip(a, b)):
            np.testing.assert_array_equal(ai, bi, err_msg=f"{what} output {k}")
        if what[0] == "lanczos" and what[1] == 10:
            P.check_lanczos(a, 10, reorth=what[2], l2=l2)
        elif what[0] != "lanczos":
            P.check(what[0], a)
    info = X.placement_info()["lanczos"]
    assert info["timed"] == 3 and info["m"] == 10 and info["stage"] == -1 and len(info["ms"]) == 3
    assert all(ms > 0 for ms in info["ms"])
    assert info["kept"] == keep if keep >= 0 else 0 <= info["kept"] < 3
    lb = B.placement_info()["lanczos"]
    assert lb["timed"] == 0 and lb["stage"] == 0


@pytest.mark.parametrize("keep", [-1, 0, 2])
@pytest.mark.parametrize("kind", sorted(SEARCH))
def test_lanczos_search(kind, keep):
    name, step = SEARCH[kind]
    P = problem(name)
    X = P.handle(3, keep)
    check_search(P, X, keep, step)
    expect_format(X, name)
    assert X.placement_info()["probed"] == 3


def test_lanczos_search_l2():
    P = problem("win_jag")
    check_search(P, P.handle(3, 2), 2, "early", l2=L2)


@pytest.mark.parametrize("name,step", [("win_jag_f32", None), ("sorted8_f32", "fused-sorted")])
def test_lanczos_search_fp32(name, step):
    P = problem(name)
    check_search(P, P.handle(3, 2), 2, step)


# ------------------------------------------------------ d. search interrupted
def searching_handle(P, keep=2):
    """A handle two timed calls into its search: two candidate placements alive, the second applied."""
    X = P.handle(3, keep)
    for call in range(3):
        out = P.lanczos(X, 10)
        for a, b in zip(out, P.base("lanczos")):
            np.testing.assert_array_equal(a, b)
    info = X.placement_info()["lanczos"]
    assert info["timed"] == 2 and info["stage"] == 3 and info["kept"] == -1
    return X


@pytest.mark.parametrize("name,other,fmt", [("sorted8", "wave", WAVE), ("win_acc", "win_jag", None)])
def test_search_interrupted_by_a_rebuild(name, other, fmt):
    P, Q = problem(name), problem(other)
    X = searching_handle(P)
    if fmt is None:   # the same padded matrix: pass 2 from window-accum to jagged
        X.set_pass_format(1, WINDOW)
        X.set_pass_format(2, JAG)
    else:
        X.set_slicing(1)
        X.set_format(fmt)
    Q.check_both(X, "lanczos", "after the rebuild:")
    expect_format(X, other)
    info = X.placement_info()
    assert info["probed"] == 3 and info["kept"] == 2
    assert info["lanczos"]["timed"] == 0 and info["lanczos"]["stage"] == 1 and info["lanczos"]["kept"] == -1
    for timed in (1, 2, 3):
        Q.check_both(X, "lanczos")
        assert X.placement_info()["lanczos"]["timed"] == timed
    assert X.placement_info()["lanczos"]["stage"] == -1 and X.placement_info()["lanczos"]["kept"] == 2
    for op in ("hvp", "gradient", "lanczos"):
        Q.check_both(X, op, "after the second search:")


def test_search_interrupted_by_graph_replay():
    P = problem("win_jag")
    X = searching_handle(P)
    X.set_graph(True)
    V = torch.zeros((10, P.d), dtype=P.dtype, device=DEV)
    wd, gd = P.t(P.w), P.t(P.g)
    for call in range(4):   # eager, captured, replayed, replayed
        V.zero_()
        _, al, be, info = X.lanczos(wd, gd, 10, V=V)
        for a, b in zip([al, be, lz_info(info), h(V)], P.base("lanczos")):
            np.testing.assert_array_equal(a, b, err_msg=f"call {call} under set_graph")
        lz = X.placement_info()["lanczos"]
        assert lz["timed"] == 2 and lz["stage"] == 3
    P.check_both(X, "hvp")
    X.set_graph(False)      # the search picks up where it stopped
    P.check_both(X, "lanczos")
    lz = X.placement_info()["lanczos"]
    assert lz["timed"] == 3 and lz["stage"] == -1 and lz["kept"] == 2
    P.check_both(X, "lanczos")
    P.check_both(X, "gradient")


def test_search_interrupted_by_destroy():
    P = problem("win_jag")
    X = searching_handle(P)
    X.close()
    del X
    Y = P.handle(3, 2)
    P.check_both(Y, "hvp", "a new handle after the drop:")
    P.check_both(Y, "lanczos")
    assert_probe(Y, 3, 2)
