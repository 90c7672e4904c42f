"""Sharded handles over several virtual ranks at partition edges.

The virtual communicator (krcn_comm_create_virtual, krcn.dist.VirtualShards)
is the only way the multi-rank code runs on one GPU.  These tests drive it at
the places where N > 1 differs from N = 1 and a few hundred rows suffice:

  1. the all-reduce itself (k_virtual_sum): worlds 2, 3, 8, 16, both dtypes,
     lengths around a workgroup and past the 1024-block grid cap, byte-equal
     to the sum in rank order and equal on every rank;
  2. the objective pieces on rank blocks of 1, 255, 256 and 257 rows or
     columns (tests/shard_cases.py crafts the matrices; tests/test_shard_cases.py
     proves the cuts on the CPU): exact on integer matrices, and against a
     long-double evaluation on the whole matrix at the suite's bounds
     (1e-13 fp64, 1e-5 fp32), plus the re-agreement of row shards after a
     re-plan;
  3. the recurrence: early-rows / early-cols with m = 1, 2, 3, 10 and
     l2 = 0 / 0.01, the breakdown quirks over ranks — the column cuts of the
     breakdown fixtures leave ranks without a nonzero —, the generic step with
     fp32 handles and with reorthogonalisation on row shards;
  4. Cubic_Krylov_LS (host step) over 2 and 3 ranks by rows and by columns.

Every replicated result must have the same bytes on every rank: ranks that
disagree by one bit in alpha, beta or a flag take different branches, and a
real communicator then deadlocks.

Shape of every test: each rank's function issues the same calls in the same
order and only returns values; what a single rank could refuse (the partition,
the step, reservations) is settled before the threads start; every assertion
runs after the ranks have returned.  Each figure is printed ("MEASURED ...")
before it is asserted.
"""
import concurrent.futures as cf

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import krcn_oracle as O
import shard_cases as SC
from conftest import golden_csr, rel_err
from krcn import _lib
from krcn import dist as kdist
from krcn import synth
from optimizer.cubic import Cubic_Krylov_LS
from optimizer.loss import LogisticRegression

pytestmark = pytest.mark.gpu

DTYPES = {"fp64": (np.float64, torch.float64, 1e-13), "fp32": (np.float32, torch.float32, 1e-5)}
WORLDS = (2, 3, 8)
N_, D_ = _lib.KRCN_SPACE_N, _lib.KRCN_SPACE_D


def device():
    return torch.device("cuda", torch.cuda.current_device())


def measured(section, name, value, bound):
    print(f"MEASURED {section} {name} {value:.3e} bound {bound:.0e}")
    return value


def within(section, name, got, ref, bound):
    e = measured(section, name, rel_err(got, ref), bound)
    assert e < bound, f"{section} {name}: {e:.3e} >= {bound:.0e}"


def scalar_within(section, name, got, ref, bound):
    ref = float(ref)
    e = measured(section, name, abs(got - ref) / max(abs(ref), 1e-300), bound)
    assert abs(got - ref) <= bound * abs(ref), f"{section} {name}: {got!r} against {ref!r}"


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def dv(X, a):
    """A host vector on X's device in X's dtype."""
    return torch.from_numpy(np.ascontiguousarray(a)).to(X.device, X.dtype)


class Cut:
    """A VirtualShards' partition applied to whole host vectors and rank results."""

    def __init__(self, vs):
        self.mode, self.bounds, self.world = vs.mode, [int(v) for v in vs.bounds], vs.world

    def _blk(self, a, r):
        return a[self.bounds[r]:self.bounds[r + 1]]

    def n(self, a, r):
        return self._blk(a, r) if self.mode == "rows" else a

    def d(self, a, r):
        return self._blk(a, r) if self.mode == "cols" else a

    def whole(self, space, parts, name, axis=0):
        """The global vector from the ranks' results: the blocks side by side
        where `space` is the cut one, else any rank's — after checking that
        every rank holds the same bytes."""
        if (space == "n") == (self.mode == "rows"):
            return np.concatenate(parts, axis=axis)
        for r, p in enumerate(parts):
            assert same_bytes(p, parts[0]), f"{name}: rank {r} differs from rank 0 ({self.mode} x {self.world})"
        return parts[0]


def agree(values, name):
    """Host scalars (or small arrays) of every rank: the same bytes."""
    first = np.asarray(values[0])
    for r, v in enumerate(values):
        assert same_bytes(np.asarray(v), first), f"{name}: rank {r} holds {v!r}, rank 0 {values[0]!r}"
    return values[0]


# ======================================================================
# 1. the all-reduce
# ======================================================================
COUNTS = (0, 1, 255, 256, 257, 256 * 1024 + 1)   # a workgroup is 256 wide, the grid capped at 1024 blocks
CANARIES = 64


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("world", [2, 3, 8, 16])
def test_virtual_allreduce(world, dtype):
    """krcn_comm_allreduce on a virtual group: one host thread and one stream
    per rank.  k_virtual_sum only adds, ((b0 + b1) + b2) + ..., so every rank's
    result is byte-equal to numpy's sum in that order and dtype; the 64 NaNs
    past the count stay; count 0 touches nothing."""
    npdt, tdt, _ = DTYPES[dtype]
    dev = device()
    rng = np.random.default_rng(1000 * world + (dtype == "fp32"))
    comms = kdist.Communicator.virtual(world, dev)
    streams = [torch.cuda.Stream(dev) for _ in range(world)]
    runs = []
    try:
        with cf.ThreadPoolExecutor(max_workers=world) as ex:
            for count in COUNTS:
                # magnitudes over ten binades: the sum depends on its order
                host = [np.concatenate([(rng.uniform(-1, 1, count) * np.exp(rng.uniform(-5, 5, count))).astype(npdt),
                                        np.full(CANARIES, np.nan, dtype=npdt)]) for _ in range(world)]
                bufs = [torch.from_numpy(h).to(dev) for h in host]
                torch.cuda.synchronize(dev)

                def one(r, bufs=bufs, count=count):
                    torch.cuda.set_device(dev)
                    with torch.cuda.stream(streams[r]):
                        comms[r].allreduce_(bufs[r][:count])
                        streams[r].synchronize()
                        return bufs[r].cpu().numpy()

                futs = [ex.submit(one, r) for r in range(world)]
                cf.wait(futs)
                runs.append((count, host, [f.result() for f in futs]))
    finally:
        for c in comms:
            c.close()
    for count, host, res in runs:
        want = host[0][:count].copy()
        for r in range(1, world):
            want = want + host[r][:count]
        assert want.dtype == npdt
        for r in range(world):
            assert res[r].dtype == npdt and res[r].shape == (count + CANARIES,)
            assert same_bytes(res[r][count:], host[r][count:]), f"count {count}: rank {r}'s canaries changed"
            assert same_bytes(res[r][:count], res[0][:count]), f"count {count}: rank {r} differs from rank 0"
            bad = np.flatnonzero(res[r][:count] != want)
            assert same_bytes(res[r][:count], want), \
                f"count {count}: rank {r} differs from the rank-order sum at {bad[:5]} ({len(bad)} places)"


# ======================================================================
# 2. objective pieces over ranks
# ======================================================================
CRAFTED = [(sizes, mode) for mode in ("rows", "cols") for sizes in SC.EDGE_SIZES]


def crafted_id(case):
    return f"{case[1]}-{SC.size_id(case[0])}"


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("case", CRAFTED, ids=crafted_id)
def test_layout_exact_on_integer_matrices(case, dtype):
    """matvec, rmatvec and hvp(l2 = 0) on the integer variant with integer
    vectors: every product and partial sum is an integer below 2^24
    (tests/test_shard_cases.py), so no order of the sums — in a kernel or over
    the ranks — changes a bit, the one division by n rounds once on both
    sides, and the results must be the bytes numpy gets on the whole matrix.
    A block placed one row off, a tail element summed or dropped, or a rank
    summed twice cannot hide in rounding: every rank's block has an entry in
    the first and in the last row (column) of the uncut dimension, the
    vectors hold no zero and the weights' ends are 4, so the elements at the
    ends of every all-reduce carry a term from every rank."""
    sizes, mode = case
    npdt, tdt, _ = DTYPES[dtype]
    A = SC.crafted_case(sizes, mode, seed=11, integer=True)
    n, d = A.shape
    x, v, u, w = SC.integer_inputs(n, d)
    vs = kdist.VirtualShards(A, SC.labels(n, 5), len(sizes), partition=mode, dtype=tdt)
    try:
        assert vs.mode == mode and list(np.diff(vs.bounds)) == list(sizes)
        cut = Cut(vs)

        def fn(r):
            X = vs.X[r]
            Ax = X.matvec(dv(X, cut.d(x, r)))
            y = X.rmatvec(dv(X, cut.n(u, r)))
            hv = X.hvp(dv(X, cut.n(w, r)), dv(X, cut.d(v, r)))
            return Ax.cpu().numpy(), y.cpu().numpy(), hv.cpu().numpy()

        res = vs.run(fn)
    finally:
        vs.close()
    Ax = cut.whole("n", [r[0] for r in res], "matvec")
    y = cut.whole("d", [r[1] for r in res], "rmatvec")
    hv = cut.whole("d", [r[2] for r in res], "hvp")
    want = {"matvec": (Ax, (A @ x).astype(npdt)),
            "rmatvec": (y, (A.T @ u).astype(npdt) / npdt(n)),
            "hvp": (hv, (A.T @ (w * (A @ v))).astype(npdt) / npdt(n))}
    for name, (got, ref) in want.items():
        assert got.dtype == ref.dtype == npdt and got.shape == ref.shape, name
        bad = np.flatnonzero(got != ref)
        assert same_bytes(got, ref), f"{name}: {len(bad)} entries differ, first at {bad[:5]}: {got[bad[:5]]} against {ref[bad[:5]]}"


VALUE_CASES = [("crafted", sizes, mode) for sizes, mode in CRAFTED] + \
              [("f1", world, mode) for mode in ("rows", "cols") for world in WORLDS]


def value_case_id(case):
    return f"{case[0]}-{case[2]}-{SC.size_id(case[1]) if case[0] == 'crafted' else case[1]}"


def longdouble_reference(A, b01, x, xs, v, l2):
    """The objective pieces on the whole matrix in np.longdouble (dense: the
    cases are a few hundred rows)."""
    L = np.longdouble
    Ad = A.toarray().astype(L)
    n = L(A.shape[0])
    b01, x, v = b01.astype(L), x.astype(L), v.astype(L)

    def loss(xx):
        z = Ad @ xx.astype(L)
        return np.mean((1 - b01) * z + np.logaddexp(L(0), -z))

    z = Ad @ x
    s = 1 / (1 + np.exp(-z))
    w = s * (1 - s)
    g = Ad.T @ (s - b01) / n
    return {"Ax": z, "w": w, "g": g, "g_l2": g + L(l2) * x, "loss": loss(x), "losses": [loss(xx) for xx in xs],
            "hvp_l2": Ad.T @ (w * (Ad @ v)) / n + L(l2) * v}


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("case", VALUE_CASES, ids=value_case_id)
def test_objective_values_over_ranks(f1, case, dtype):
    """weights, gradient (l2 = 0 and 0.01), loss_mean, loss_values (k = 3),
    hvp (l2 = 0.01), dot and diff_norm in both spaces against a long-double
    evaluation on the whole matrix: rel 1e-13 (fp64) / 1e-5 (fp32, from the
    fp32-rounded inputs), the suite's bounds for these pieces.  Replicated
    vectors and every host scalar must have the same bytes on all ranks.  The
    dot operands are a and 0.5 a + 0.1 noise, so the dot does not cancel and
    a relative bound on it means what it says."""
    kind, arg, mode = case
    npdt, tdt, tol = DTYPES[dtype]
    sec = f"s2-{dtype}"
    if kind == "crafted":
        A, world = SC.crafted_case(arg, mode, seed=12), len(arg)
        b = SC.labels(A.shape[0], 5)
    else:
        A, world, b = golden_csr(f1), arg, f1["b"]
    # the reference sees the values the handle holds
    A = sp.csr_matrix((A.data.astype(npdt).astype(np.float64), A.indices, A.indptr), shape=A.shape)
    n, d = A.shape
    rng = np.random.default_rng(77)
    rnd = lambda k, s=1.0: (s * rng.uniform(-1, 1, k)).astype(npdt).astype(np.float64)  # noqa: E731
    x, v, l2 = rnd(d, 0.5), rnd(d), 0.01
    xs = [rnd(d, 0.5) for _ in range(3)]
    ad, an = rnd(d), rnd(n)
    bd = (0.5 * ad + rnd(d, 0.1)).astype(npdt).astype(np.float64)
    bn = (0.5 * an + rnd(n, 0.1)).astype(npdt).astype(np.float64)
    vs = kdist.VirtualShards(A, b, world, partition=mode, dtype=tdt)
    try:
        assert vs.mode == mode
        if kind == "crafted":
            assert list(np.diff(vs.bounds)) == list(arg)
        cut = Cut(vs)

        def fn(r):
            X, br = vs.X[r], vs.b[r]
            xd = dv(X, cut.d(x, r))
            Ax = X.matvec(xd)
            w = X.weights(Ax)
            g = X.gradient(Ax, br)
            g_l2 = X.gradient(Ax, br, xd, l2=l2)
            loss = X.loss_mean(Ax, br)
            losses = X.loss_values([dv(X, cut.d(xx, r)) for xx in xs], br)
            hv = X.hvp(w, dv(X, cut.d(v, r)), l2=l2)
            a_d, b_d, a_n, b_n = dv(X, cut.d(ad, r)), dv(X, cut.d(bd, r)), dv(X, cut.n(an, r)), dv(X, cut.n(bn, r))
            scalars = {"dot_d": X.dot(a_d, b_d, D_), "dot_n": X.dot(a_n, b_n, N_),
                       "norm_d": X.diff_norm(a_d, space=D_), "norm_n": X.diff_norm(a_n, space=N_),
                       "diff_d": X.diff_norm(a_d, b_d, D_), "diff_n": X.diff_norm(a_n, b_n, N_)}
            return {"Ax": Ax.cpu().numpy(), "w": w.cpu().numpy(), "g": g.cpu().numpy(), "g_l2": g_l2.cpu().numpy(),
                    "hvp_l2": hv.cpu().numpy(), "loss": loss, "losses": losses, "scalars": scalars}

        res = vs.run(fn)
    finally:
        vs.close()
    ref = longdouble_reference(A, np.asarray(O.labels01(b), dtype=np.float64), x, xs, v, l2)
    for name, space in (("Ax", "n"), ("w", "n"), ("g", "d"), ("g_l2", "d"), ("hvp_l2", "d")):
        got = cut.whole(space, [r[name] for r in res], name)
        assert got.dtype == npdt
        within(sec, name, got, ref[name], tol)
    scalar_within(sec, "loss_mean", agree([r["loss"] for r in res], "loss_mean"), ref["loss"], tol)
    losses = agree([r["losses"] for r in res], "loss_values")
    assert len(losses) == 3
    for k in range(3):
        scalar_within(sec, f"loss_values[{k}]", losses[k], ref["losses"][k], tol)
    L = np.longdouble
    want = {"dot_d": ad.astype(L) @ bd.astype(L), "dot_n": an.astype(L) @ bn.astype(L),
            "norm_d": np.sqrt(ad.astype(L) @ ad.astype(L)), "norm_n": np.sqrt(an.astype(L) @ an.astype(L)),
            "diff_d": np.sqrt(np.sum((ad.astype(L) - bd.astype(L)) ** 2)),
            "diff_n": np.sqrt(np.sum((an.astype(L) - bn.astype(L)) ** 2))}
    for name, w_ref in want.items():
        scalar_within(sec, name, agree([r["scalars"][name] for r in res], name), w_ref, tol)


def info_fields(info):
    return (info.m_eff, info.breakdown, info.j_break, info.hvps, info.beta_last, info.gnorm)


def golden_lanczos_checks(sec, tag, V, al, be, info, ref, gnorm_ref, v_tol=1e-6):
    """One recurrence against (V d x m_eff, alphas, betas, beta) at the suite's
    golden tolerances (tests/test_gpu_lanczos.py::test_lanczos_vs_golden)."""
    Vr, al_r, be_r, beta_r = ref
    m_eff, _, _, _, beta_last, gnorm = info
    assert m_eff == Vr.shape[1] == len(al), tag
    assert al.shape == al_r.shape and be.shape == be_r.shape, tag
    within(sec, f"{tag} alphas", al, al_r, 1e-11)
    within(sec, f"{tag} betas", be, be_r, 1e-11)
    e = measured(sec, f"{tag} V", float(np.abs(V[:m_eff].T - Vr).max()), v_tol)
    assert e < v_tol, tag
    measured(sec, f"{tag} beta_last", abs(beta_last - float(beta_r)) / max(abs(float(beta_r)), 1e-300), 1e-11)
    assert abs(beta_last - float(beta_r)) <= 1e-11 * max(1e-300, abs(float(beta_r))), tag
    measured(sec, f"{tag} gnorm", abs(gnorm - gnorm_ref) / gnorm_ref, 1e-13)
    assert abs(gnorm - gnorm_ref) <= 1e-13 * gnorm_ref, tag


def test_row_shards_agree_again_after_a_replan():
    """Rows (1, 256, 257): every rank thread re-plans twice (sorted tiles,
    then 8 slices; each re-plan ends in the collective agree_rows through
    krcn_csr_reserve) and reserves m = 10.  The ranks must then report one
    step, and the m = 10 recurrence must match the oracle.  The new plans'
    slice combines write one alpha partial on the blocks of 1 and 256 rows
    and two on the block of 257, so the packed tail of the step's all-reduce
    is the agreed two and the shorter ranks zero-fill theirs."""
    sizes, m = (1, 256, 257), 10
    A = SC.crafted_case(sizes, "rows", seed=12)
    b = SC.labels(A.shape[0], 5)
    vs = kdist.VirtualShards(A, b, len(sizes), partition="rows")
    try:
        assert list(np.diff(vs.bounds)) == list(sizes)
        before = [X.plan_info() for X in vs.X]

        def fn(r):
            X = vs.X[r]
            X.set_format(_lib.KRCN_FORMAT_SORTED)
            X.set_slicing(8)
            X.reserve(m)
            step, plan = X.lanczos_step(), X.plan_info()
            Ax = X.matvec(torch.full((X.d,), 0.5, dtype=X.dtype, device=X.device))
            g = X.gradient(Ax, vs.b[r])
            V, al, be, info = X.lanczos(X.weights(Ax), g, m)
            return step, plan, V.cpu().numpy()[:info.m_eff], al, be, info_fields(info), g.cpu().numpy()

        res = vs.run(fn)
    finally:
        vs.close()
    for r, out in enumerate(res):
        assert out[1] != before[r], f"rank {r} kept its plans"
        assert out[1]["pass1"][0] == -8, out[1]    # sorted tiles over 8 slices
    assert agree([out[0] for out in res], "lanczos_step") == "early-rows"
    x = np.full(A.shape[1], 0.5)
    gh = O.gradient(A, O.labels01(b), x)
    wh = O.hessian_weights(A, x)
    ref = O.lanczos(lambda z: O.hvp_from_weights(A, wh, z), gh, m)
    cut = Cut(vs)
    V = cut.whole("d", [out[2] for out in res], "V", axis=1)
    within("s2-replan", "gradient", cut.whole("d", [out[6] for out in res], "g"), gh, 1e-13)
    golden_lanczos_checks("s2-replan", "m10", V, agree([out[3] for out in res], "alphas"),
                          agree([out[4] for out in res], "betas"), agree([out[5] for out in res], "info"), ref,
                          float(np.linalg.norm(gh)))


# ======================================================================
# 3. the recurrence over ranks
# ======================================================================
EARLY = {"rows": "early-rows", "cols": "early-cols"}
SHARDINGS = [(mode, world) for mode in ("rows", "cols") for world in WORLDS]


def sharding_id(s):
    return f"{s[0]}x{s[1]}"


def run_recurrences(vs, x, calls):
    """On every rank: the gradient at x, then lanczos(w, g, **kw) for every kw
    of `calls`.  Returns (cut, g, [(V, alphas, betas, info fields) per call])
    with V (its m_eff basis rows; the rows past them are not part of the
    result) and g assembled over the ranks and the replicated results checked
    to be the same bytes on every rank."""
    cut = Cut(vs)

    def fn(r):
        X = vs.X[r]
        Ax = X.matvec(dv(X, cut.d(x, r)))
        w = X.weights(Ax)
        g = X.gradient(Ax, vs.b[r])
        out = []
        for kw in calls:
            V, al, be, info = X.lanczos(w, g, **kw)
            out.append((V.cpu().numpy()[:info.m_eff], al, be, info_fields(info)))
        return g.cpu().numpy(), out

    res = vs.run(fn)
    g = cut.whole("d", [r[0] for r in res], "gradient")
    runs = []
    for k, kw in enumerate(calls):
        info = agree([r[1][k][3] for r in res], f"info {kw}")
        V = cut.whole("d", [r[1][k][0] for r in res], f"V {kw}", axis=1)
        runs.append((V, agree([r[1][k][1] for r in res], f"alphas {kw}"), agree([r[1][k][2] for r in res], f"betas {kw}"),
                     info))
    return cut, g, runs


def f2_reference(f2, A, wh, m):
    """The golden recurrence of f1's operator with l2 = 0 for m steps.  The
    fixture holds m = 1 and m = 10; m = 2, 3 come from the oracle, which
    tests/test_oracle_golden.py pins to the fixture bit for bit and whose
    first m - 1 alphas, betas and m basis vectors are the fixture's m = 10
    prefix (checked here)."""
    if f"alphas_m{m}" in f2.files:
        return f2[f"V_m{m}"], f2[f"alphas_m{m}"], f2[f"betas_m{m}"], f2[f"beta_m{m}"]
    V, al, be, beta = O.lanczos(lambda z: O.hvp_from_weights(A, wh, z), f2["g"], m)
    assert same_bytes(al[:m - 1], f2["alphas_m10"][:m - 1]) and same_bytes(be, f2["betas_m10"][:m - 1])
    assert same_bytes(V, f2["V_m10"][:, :m])
    return V, al, be, beta


@pytest.mark.parametrize("sharding", SHARDINGS, ids=sharding_id)
def test_early_steps_over_ranks(f1, f2, sharding):
    """fp64, no reorthogonalisation: the single-collective steps.  m = 1 runs
    no loop step, m = 2 only the j = 0 launch (an all-reduce of n, the final
    globalise), m = 3 adds the first j > 0 step (n + 2 on column shards) and
    m = 10 the steady state.  l2 = 0 against the golden recurrence, l2 = 0.01
    against the oracle over hvp_from_weights(.., l2): alphas, betas 1e-11,
    V 1e-6 (f1's operator moves V[:, 9] by 8e-9 under a 1e-16 perturbation),
    beta_last 1e-11, gnorm 1e-13."""
    mode, world = sharding
    A, ms, l2s = golden_csr(f1), (1, 2, 3, 10), (0.0, 0.01)
    calls = [dict(m=m, l2=l2) for l2 in l2s for m in ms]
    vs = kdist.VirtualShards(A, f1["b"], world, partition=mode)
    try:
        steps = [X.lanczos_step() for X in vs.X]
        cut, g, runs = run_recurrences(vs, f1["x0"], calls)
    finally:
        vs.close()
    assert steps == [EARLY[mode]] * world
    sec = f"s3-early-{mode}"
    within(sec, "gradient", g, f1["grad0"], 1e-13)
    wh = O.hessian_weights(A, f1["x0"])
    gnorm = float(np.linalg.norm(f2["g"]))
    for kw, (V, al, be, info) in zip(calls, runs):
        m, l2 = kw["m"], kw["l2"]
        if l2 == 0.0:
            ref = f2_reference(f2, A, wh, m)
        else:
            ref = O.lanczos(lambda z: O.hvp_from_weights(A, wh, z, l2=l2), f2["g"], m)
        assert info[1] == 0 and info[3] == m, (kw, info)   # no breakdown, m HVPs
        golden_lanczos_checks(sec, f"x{world} m{m} l2={l2}", V, al, be, info, ref, gnorm)


@pytest.mark.parametrize("sharding", SHARDINGS, ids=sharding_id)
@pytest.mark.parametrize("r,ms", [(1, (2, 3, 5)), (3, (4, 5, 10))])
def test_breakdown_quirks_over_ranks(f2, r, ms, sharding):
    """tests/test_gpu_lanczos.py::test_lanczos_breakdown_quirks over ranks, at
    its tolerances.  The column cuts give ranks blocks without a nonzero
    (r1: all ranks but the first; r3 x 8: five of eight —
    tests/test_shard_cases.py): such a rank still reaches every collective of
    the recurrence with zeros in hand."""
    mode, world = sharding
    A = golden_csr(f2, f"r{r}_")
    calls = [dict(m=m) for m in ms]
    vs = kdist.VirtualShards(A, f2[f"r{r}_b"], world, partition=mode)
    try:
        steps = [X.lanczos_step() for X in vs.X]
        nnz = [X.nnz for X in vs.X]
        cut, g, runs = run_recurrences(vs, np.full(A.shape[1], 0.5), calls)
    finally:
        vs.close()
    assert steps == [EARLY[mode]] * world
    if mode == "cols" and (r, world) != (3, 2) and (r, world) != (3, 3):
        assert min(nnz) == 0, nnz
    sec = f"s3-breakdown-{mode}"
    within(sec, f"r{r} x{world} gradient", g, f2[f"r{r}_g"], 1e-13)
    for kw, (V, al, be, info) in zip(calls, runs):
        m = kw["m"]
        key = f"r{r}_m{m}"
        Vref = f2[f"{key}_V"]
        m_eff, breakdown, j_break, _, beta_last, _ = info
        assert breakdown == 1 and j_break == r - 1, (key, info)
        assert m_eff == Vref.shape[1]
        assert al.shape == f2[f"{key}_alphas"].shape and be.shape == f2[f"{key}_betas"].shape
        within(sec, f"{key} x{world} alphas", al, f2[f"{key}_alphas"], 1e-11)
        measured(sec, f"{key} x{world} betas", rel_err(be, f2[f"{key}_betas"]), 1e-11)
        np.testing.assert_allclose(be, f2[f"{key}_betas"], rtol=1e-11, atol=0)
        Vh = V[:m_eff].T
        e = measured(sec, f"{key} x{world} V", float(np.abs(Vh - Vref).max()), 1e-12)
        assert e < 1e-12
        if m == r + 1:   # breakdown at j == m - 2: the zero last column is kept
            assert np.all(Vh[:, -1] == 0) and be[-1] == 0
        assert beta_last < 1e-6


@pytest.mark.parametrize("sharding", SHARDINGS, ids=sharding_id)
def test_generic_step_fp32_over_ranks(f1, sharding):
    """fp32 handles run the generic step (the early steps are fp64 only): its
    all-reduces carry fp32 vectors and its d-space dots are made global one
    scalar at a time.  m = 10 on f1; the leading six alphas and betas against
    the fp64 oracle at 1e-3, the suite's fp32 recurrence bound."""
    mode, world = sharding
    A, m = golden_csr(f1), 10
    vs = kdist.VirtualShards(A, f1["b"], world, partition=mode, dtype=torch.float32)
    try:
        steps = [X.lanczos_step() for X in vs.X]
        cut, g, runs = run_recurrences(vs, f1["x0"], [dict(m=m)])
    finally:
        vs.close()
    assert steps == ["generic"] * world
    sec = f"s3-fp32-{mode}"
    within(sec, f"x{world} gradient", g, f1["grad0"], 1e-5)
    wh = O.hessian_weights(A, f1["x0"])
    _, al_r, be_r, _ = O.lanczos(lambda z: O.hvp_from_weights(A, wh, z), f1["grad0"], m)
    V, al, be, info = runs[0]
    assert V.dtype == np.float32 and info[0] == m and info[1] == 0
    within(sec, f"x{world} alphas[:6]", al[:6], al_r[:6], 1e-3)
    within(sec, f"x{world} betas[:6]", be[:6], be_r[:6], 1e-3)


@pytest.mark.parametrize("world", WORLDS)
def test_reorthogonalised_recurrence_on_row_shards(world):
    """reorth=True on row shards (the d-space sweeps of CGS2 are replicated,
    the HVP's d-vector all-reduced): the matrix, m = 40 and the bounds of
    tests/test_gpu_cgs2.py::test_recurrence_column_sharded_on_two_virtual_ranks
    — alphas / betas against the oracle's CGS2 at 1e-10, V orthonormal to
    1e-12 —, and V, alphas, betas the same bytes on every rank."""
    A, b = synth.make_problem(None, seed=7, n=400, d=101, nnz=6000)
    m = 40
    vs = kdist.VirtualShards(A, b, world, partition="rows")
    try:
        for X in vs.X:   # no collective: the plans exist and the ranks have agreed (attach)
            X.reserve(m, reorth=True)
        steps = [X.lanczos_step(reorth=True) for X in vs.X]
        cut, g, runs = run_recurrences(vs, np.full(A.shape[1], 0.5), [dict(m=m, reorth=True)])
    finally:
        vs.close()
    assert steps == ["generic"] * world
    x = np.full(A.shape[1], 0.5)
    wh = O.hessian_weights(A, x)
    gh = O.gradient(A, O.labels01(b), x)
    sec = "s3-reorth-rows"
    within(sec, f"x{world} gradient", g, gh, 1e-13)
    _, al_r, be_r, _ = O.lanczos_cgs2(lambda z: O.hvp_from_weights(A, wh, z), gh, m)
    V, al, be, info = runs[0]
    assert info[0] == m == len(al_r)
    within(sec, f"x{world} alphas", al, al_r, 1e-10)
    within(sec, f"x{world} betas", be, be_r, 1e-10)
    e = measured(sec, f"x{world} orthonormality", float(np.abs(V @ V.T - np.eye(m)).max()), 1e-12)
    assert e < 1e-12


# ======================================================================
# 4. the optimizer over ranks
# ======================================================================
@pytest.fixture(scope="module")
def f4_problem(f4):
    n, d, nnz = (int(v) for v in f4["shape"])
    return synth.make_problem(None, seed=int(f4["seed"]), n=n, d=d, nnz=nnz)


@pytest.mark.parametrize("sharding", [(mode, world) for mode in ("rows", "cols") for world in (2, 3)],
                         ids=sharding_id)
def test_krylov_crn_over_ranks(f4, f4_problem, sharding):
    """Cubic_Krylov_LS (host step) for 3 steps on the trajectory fixture's
    problem, one LogisticRegression(shard=...) per rank thread: on column
    shards x and the basis are sharded, basis_combine runs on rank blocks, the
    d-space norms are summed over ranks and the convergence flag is
    rank-wide.  x_k and f_k against the fixture's first four entries at its
    1e-10; the iteration counts, the subproblem's iteration counts and
    reg_coef equal on every rank."""
    mode, world = sharding
    A, b = f4_problem
    steps = 3
    dev = device()
    got_mode, bounds = kdist.plan(A, world, mode)
    assert got_mode == mode
    comms = kdist.Communicator.virtual(world, dev)
    specs = [kdist.ShardSpec(A, mode, bounds, r, world, comms[r]) for r in range(world)]
    streams = [torch.cuda.Stream(dev) for _ in range(world)]

    def one(r):
        torch.cuda.set_device(dev)
        with torch.cuda.stream(streams[r]):
            loss = LogisticRegression(A, b, l1=0, l2=0, store_mat_vec_prod=True, shard=specs[r])
            opt = Cubic_Krylov_LS(loss=loss, reg_coef=1e-3, label="k", subspace_dim=10, tolerance=1e-9, tqdm=False)
            tr = opt.run(x0=np.full(A.shape[1], 0.5), it_max=steps)
            opt.compute_loss_of_iterates()
            out = (np.array([np.array(x) for x in tr.xs]), np.array(tr.loss_vals), list(tr.its), list(tr.solver_its),
                   opt.reg_coef, loss.device_matrix.lanczos_step())
            loss.device_matrix.close()
            return out

    try:
        with cf.ThreadPoolExecutor(max_workers=world) as ex:
            futs = [ex.submit(one, r) for r in range(world)]
            cf.wait(futs)
        res = [fu.result() for fu in futs]
    finally:
        for c in comms:
            c.close()
    k = steps + 1
    if mode == "cols":
        xs = np.concatenate([r[0] for r in res], axis=1)
    else:
        xs = agree([r[0] for r in res], "iterates")
    sec = f"s4-{mode}"
    assert xs.shape == (k, A.shape[1])
    within(sec, f"x{world} xs", xs, f4["xs"][:k], 1e-10)
    lv = agree([r[1] for r in res], "loss_vals")
    measured(sec, f"x{world} loss_vals", float(np.abs(lv / f4["loss_vals"][:k] - 1).max()), 1e-10)
    np.testing.assert_allclose(lv, f4["loss_vals"][:k], rtol=1e-10)
    assert agree([r[2] for r in res], "its") == list(range(k))
    assert agree([r[3] for r in res], "solver_its") == list(f4["solver_its"][:k])
    agree([r[4] for r in res], "reg_coef")
    assert [r[5] for r in res] == [EARLY[mode]] * world
