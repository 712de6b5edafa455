"""The damped step where a Cholesky goes wrong -- near-singular, rank-deficient and badly scaled systems -- against an mpmath reference, and the step's lifecycle.

The reference assembles A, b, c from the same [F, 122] f64 records (DenseLinearSystemBuilder, as helpers.host_system), applies buildDampedSystem's rule in 50 digits and
factors the damped matrix A~ recording every pivot.  rho = min_p pivot_p / A~_pp is the rule of include/gtsam_points_hip.h (GP_ERROR_INDETERMINATE): at or below 1e-11 the
system is indeterminate.  With a margin around it: rho >= 1e-9 -> every form solves, to 64 n eps kappa_2(A~) of the exact x; rho <= 1e-13 -> every form reports
GP_ERROR_INDETERMINATE; (case, lambda, ordering) combinations in between are not asserted on, and the generator keeps them rare (checked below).  The elimination order is the
form's own: slot order for the dense step, the symbolic phase's permutation for each sparse ordering."""
import ctypes as C

import numpy as np
import pytest

from helpers import host_system

pytestmark = pytest.mark.gpu

mpmath = pytest.importorskip("mpmath")
mp = mpmath.mp

GP_OK, GP_ERROR_INVALID_ARGUMENT, GP_ERROR_INDETERMINATE = 0, 1, 5
SOLVES, INDETERMINATE = 1e-9, 1e-13  # the margin around the library's 1e-11
ORDERINGS = ["natural", "nd", "amd", "amd1", "auto"]
LAMBDAS = [0.0, 1e-5, 1.0, 1e5]
EPS = np.finfo(np.float64).eps


# ---- the reference ---------------------------------------------------------------------------------------------------------------------------------------------------------
def mp_system(records, slots, n_slots, lam, diagonal, min_diag, max_diag, prior):
    """A~ (damped), b, c in mpmath: the assembly of helpers.host_system, exact sums of the f64 entries, then buildDampedSystem (+ prior)"""
    n = 6 * n_slots
    A = mp.zeros(n, n)
    b = [mp.mpf(0)] * n
    c = mp.mpf(0)
    for rec, (st, ss) in zip(records, slots):
        Ht, Hs, Hts = rec[2:38].reshape(6, 6).T, rec[38:74].reshape(6, 6).T, rec[74:110].reshape(6, 6).T
        c += mp.mpf(float(rec[1]))
        for s, H, g in ((st, Ht, rec[110:116]), (ss, Hs, rec[116:122])):
            if s < 0:
                continue
            for r in range(6):
                b[6 * s + r] -= mp.mpf(float(g[r]))
                for q in range(6):
                    A[6 * s + r, 6 * s + q] += mp.mpf(float(H[r, q]))
        if st >= 0 and ss >= 0:
            for r in range(6):
                for q in range(6):
                    v = mp.mpf(float(Hts[r, q]))
                    A[6 * st + r, 6 * ss + q] += v
                    A[6 * ss + q, 6 * st + r] += v
    for i in range(n):
        d = A[i, i]
        add = lam * min(max(d, mp.mpf(min_diag)), mp.mpf(max_diag)) if diagonal else mp.mpf(lam)
        if prior is not None:
            add += mp.mpf(float(prior[i]))
        A[i, i] = d + add
    return A, b, c


def mp_cholesky(A, order):
    """Cholesky of A in the elimination order `order` (slot list): -> (L or None when a pivot is not positive, rho = min pivot / A_pp)"""
    idx = [6 * s + r for s in order for r in range(6)]
    n = len(idx)
    L = mp.zeros(n, n)
    rho = mp.inf
    for j in range(n):
        d = A[idx[j], idx[j]] - mp.fsum(L[j, p] ** 2 for p in range(j))
        scale = A[idx[j], idx[j]]
        rho = min(rho, d / scale if scale > 0 else (mp.mpf(0) if d == 0 else mp.mpf(-1)))
        if d <= 0:
            return None, float(rho) if rho > -1 else -1.0
        L[j, j] = mp.sqrt(d)
        for i in range(j + 1, n):
            L[i, j] = (A[idx[i], idx[j]] - mp.fsum(L[i, p] * L[j, p] for p in range(j))) / L[j, j]
    return (L, idx), float(rho)


def mp_solve(fact, b):
    L, idx = fact
    n = len(idx)
    y = [mp.mpf(0)] * n
    for i in range(n):
        y[i] = (b[idx[i]] - mp.fsum(L[i, p] * y[p] for p in range(i))) / L[i, i]
    x = [mp.mpf(0)] * n
    for i in reversed(range(n)):
        x[i] = (y[i] - mp.fsum(L[p, i] * x[p] for p in range(i + 1, n))) / L[i, i]
    out = np.zeros(n)
    for k, i in enumerate(idx):
        out[i] = float(x[k])
    return out


class Reference:
    """everything the assertions of one (case, lambda, damping) need, computed once: x_ref, b, c, kappa_2(A~) and rho per elimination order"""

    def __init__(self, case, lam, diagonal):
        mp.dps = 50
        self.case = case
        A, b, c = mp_system(case.records, case.slots, case.P, lam, diagonal, case.min_diag, case.max_diag, case.prior)
        self.A, self.b_mp = A, b
        self.b = np.array([float(v) for v in b])
        self.c = float(c)
        self.rho = {}
        self.fact = {}
        fact, rho = mp_cholesky(A, list(range(case.P)))
        self.rho["natural"] = rho
        self.x = mp_solve(fact, b) if fact is not None else None
        Af = np.array([[float(A[i, j]) for j in range(A.cols)] for i in range(A.rows)])
        ev = np.linalg.eigvalsh(Af)
        self.kappa = float(ev[-1] / ev[0]) if ev[0] > 0 else np.inf
        # ... and of the equilibrated matrix D^-1/2 A~ D^-1/2 (D = diag A~): Cholesky's error is bounded by it in the D^1/2 norm (van der Sluis), which is what
        # says something where the poses' scales differ by 1e12 and kappa_2(A~) itself is beyond f64
        d = np.array([float(mp.sqrt(A[i, i])) if A[i, i] > 0 else 1.0 for i in range(A.rows)])
        self.d = d
        evs = np.linalg.eigvalsh(np.array([[float(A[i, j] / (mp.sqrt(A[i, i] * A[j, j]) if A[i, i] * A[j, j] > 0 else 1)) for j in range(A.cols)] for i in range(A.rows)]))
        self.kappa_eq = float(evs[-1] / evs[0]) if evs[0] > 0 else np.inf

    def rho_for(self, perm):
        key = tuple(int(p) for p in perm)
        if key not in self.rho:
            self.rho[key] = mp_cholesky(self.A, list(key))[1]
        return self.rho[key]


# ---- the cases -------------------------------------------------------------------------------------------------------------------------------------------------------------
def _rot(rng, k):
    q, r = np.linalg.qr(rng.normal(size=(k, k)))
    return q * np.sign(np.diag(r))


def _spd(rng, k, spectrum, scale=1e3):
    """V diag(spectrum) V^T, V random orthonormal: J^T J of J = U diag(s) V^T with s^2 = scale * spectrum"""
    V = _rot(rng, k)
    H = (V * (scale * np.asarray(spectrum, dtype=np.float64))) @ V.T
    return 0.5 * (H + H.T)


def _record(rng, Ht=None, Hs=None, Hts=None):
    rec = np.zeros(122)
    rec[0], rec[1] = 100, rng.uniform(1.0, 2.0)
    z = np.zeros((6, 6))
    for off, H in ((2, Ht), (38, Hs), (74, Hts)):
        rec[off : off + 36] = (z if H is None else H).T.reshape(36)  # column-major 6x6
    rec[110:122] = rng.normal(size=12) * 10.0
    return rec


def _unary(rng, M):
    """a factor whose target is held: only H_source / b_source enter (the unary HessianFactor)"""
    return _record(rng, Hs=M)


def _binary(rng, H):
    return _record(rng, Ht=H[:6, :6], Hs=H[6:, 6:], Hts=H[:6, 6:])


def _between(rng, M):
    """H = [[M, -M], [-M, M]]: exact in f64, null on (v, v) -- a relative constraint that leaves the common motion free"""
    return _record(rng, Ht=M, Hs=M, Hts=-M)


class Case:
    def __init__(self, name, P, slots, records, prior=None, min_diag=1e-6, max_diag=1e32, scalable=True):
        self.name, self.P, self.slots = name, P, [tuple(s) for s in slots]
        self.records = np.ascontiguousarray(np.asarray(records, dtype=np.float64).reshape(-1, 122))
        self.prior = None if prior is None else np.asarray(prior, dtype=np.float64)
        self.min_diag, self.max_diag = min_diag, max_diag
        self.scalable = scalable  # diagonal damping does not clip at x 1e-8 / x 1e8 (for the scaling test)

    def scaled(self, s):
        rec = self.records.copy()
        rec[:, 1:] *= s
        return Case(f"{self.name}*{s:g}", self.P, self.slots, rec, None if self.prior is None else self.prior * s, self.min_diag, self.max_diag, self.scalable)


def _chain(rng, P):
    """pose 0 held (unary factor onto slot 0), a chain of well-conditioned 12x12 factors"""
    slots, recs = [(-1, 0)], [_unary(rng, _spd(rng, 6, np.logspace(0, -1, 6)))]
    for i in range(P - 1):
        slots.append((i, i + 1))
        recs.append(_binary(rng, _spd(rng, 12, np.logspace(0, -1, 12))))
    return slots, recs


def _chain_kappa(rng, P, kappa):
    """a held pose and P poses in a chain, every constraint M = V diag(1 .. 1/kappa) V^T with ONE V (a unary M onto slot 0, between(M) on the links): A = L (x) M with L
    the chain's Laplacian + anchor, so kappa_2(A) ~ kappa x kappa(L)"""
    M = _spd(rng, 6, np.logspace(0, -np.log10(kappa), 6))
    return [(-1, 0)] + [(i, i + 1) for i in range(P - 1)], [_unary(rng, M)] + [_between(rng, M) for _ in range(P - 1)]


def make_cases():
    rng = np.random.default_rng(20261016)
    cases = []
    # condition numbers of one pose's system (unary factor with the spectrum [1 .. 1/kappa]) and of a 3-pose chain; exact rank loss (an exact zero column)
    for kappa in (1e2, 1e6, 1e9, 1e12, 1e15):
        cases.append(Case(f"one-pose-kappa{kappa:g}", 1, [(-1, 0)], [_unary(rng, _spd(rng, 6, np.logspace(0, -np.log10(kappa), 6)))]))
        slots, recs = _chain_kappa(rng, 3, kappa)
        cases.append(Case(f"chain3-kappa{kappa:g}", 3, slots, recs))
    Jz = rng.normal(size=(30, 6))
    Jz[:, 4] = 0.0
    cases.append(Case("one-pose-rank5", 1, [(-1, 0)], [_unary(rng, Jz.T @ Jz)]))
    # degenerate factors: a plane (rotation about the normal and the two in-plane translations unobservable) and a corridor (the translation along it), axis-aligned
    # (exact zeros) and rotated (rounding-level null space), one pose behind a held one and in the middle of a chain
    for name, dead in (("plane", [2, 3, 4]), ("corridor", [3])):
        J = rng.normal(size=(40, 6))
        J[:, dead] = 0.0
        M = J.T @ J
        R = np.zeros((6, 6))
        Q = _rot(rng, 3)
        R[:3, :3], R[3:, 3:] = Q, Q
        cases.append(Case(f"{name}-axis", 1, [(-1, 0)], [_unary(rng, M)], scalable=False))  # (exact zeros on the diagonal: min_diagonal clips them)
        cases.append(Case(f"{name}-rotated", 1, [(-1, 0)], [_unary(rng, R @ M @ R.T)]))
        slots, recs = _chain(rng, 3)
        recs[1] = _between(rng, M)  # the link 0 -> 1 is the degenerate one: pose 1 slides against pose 0 in the dead directions
        cases.append(Case(f"{name}-in-chain3", 3, slots, recs))
    # no pose held: relative constraints only (gauge freedom, exactly singular), and the same fixed by a prior on slot 0
    for P in (3, 12):
        slots = [(i, (i + 1) % P) for i in range(P)] + [(i, (i + 2) % P) for i in range(0, P, 3)]
        recs = [_between(rng, _spd(rng, 6, np.logspace(0, -1, 6))) for _ in slots]
        cases.append(Case(f"gauge-free-{P}", P, slots, recs))
        prior = np.zeros(6 * P)
        prior[:6] = 1e4
        cases.append(Case(f"gauge-prior-{P}", P, slots, recs, prior=prior))
    # an isolated pose (no factor touches slot 2)
    slots, recs = _chain(rng, 2)
    cases.append(Case("isolated", 3, slots, recs))
    # per-pose scale spread 1e-6 .. 1e6: D A D with D = diag(d_slot) (min_diagonal clips the small poses' diagonal under diagonal damping)
    P = 5
    slots, recs = _chain(rng, P)
    d = np.logspace(-6, 6, P)
    for k, (st, ss) in enumerate(slots):
        r = recs[k]
        for off, a, bb in ((2, st, st), (38, ss, ss), (74, st, ss)):
            if a >= 0 and bb >= 0:
                r[off : off + 36] *= d[a] * d[bb]
        if st >= 0:
            r[110:116] *= d[st]
        if ss >= 0:
            r[116:122] *= d[ss]
    cases.append(Case("scale-spread", P, slots, recs, scalable=False))
    # a well-conditioned 12-pose chain with loops (72 unknowns), and max_diagonal clipping it
    slots, recs = _chain(rng, 12)
    for i in range(0, 10, 3):
        slots.append((i, i + 2))
        recs.append(_binary(rng, _spd(rng, 12, np.logspace(0, -2, 12))))
    cases.append(Case("chain12", 12, slots, recs))
    cases.append(Case("chain12-maxclip", 12, slots, recs, max_diag=50.0, scalable=False))
    # all records scaled by 1e-8 and by 1e8
    base = [c for c in cases if c.name in ("chain3-kappa1e+06", "gauge-free-3", "plane-in-chain3")]
    for s in (1e-8, 1e8):
        cases += [c.scaled(s) for c in base]
    return cases


CASES = make_cases()
_REFS = {}


def reference(case, lam, diagonal):
    key = (case.name, lam, diagonal)
    if key not in _REFS:
        _REFS[key] = Reference(case, lam, diagonal)
    return _REFS[key]


# ---- the forms under test ----------------------------------------------------------------------------------------------------------------------------------------------------
def _step_call(lib, kind, h, rec_dev, lam, diagonal, case, halves):
    n = 6 * case.P
    x, b, c = np.full(n, np.nan), np.full(n, np.nan), np.full(1, np.nan)
    prior = case.prior.ctypes.data if case.prior is not None else None
    args = (h, C.c_void_p(rec_dev.data_ptr()), float(lam), int(diagonal), float(case.min_diag), float(case.max_diag), prior)
    if halves:
        rc = getattr(lib, f"gp_{kind}_system_issue_step")(*args)
        assert rc == GP_OK, rc
        rc = getattr(lib, f"gp_{kind}_system_finish_step")(h, x.ctypes.data, b.ctypes.data, c.ctypes.data)
    else:
        rc = getattr(lib, f"gp_{kind}_system_step")(*args, x.ctypes.data, b.ctypes.data, c.ctypes.data)
    return rc, x, b, float(c[0])


def forms(gpu, case):
    """(label, kind, handle-owner, elimination order, one_launch flag) for every form that takes this case"""
    out = []
    dense = gpu.DenseLinearSystemGPU(case.P, case.slots)
    if case.P == 1:
        out.append(("dense-one-launch", "dense", dense, [0], True))
        out.append(("dense-multi-launch", "dense", dense, [0], False))
    else:
        out.append(("dense", "dense", dense, list(range(case.P)), True))
    for o in ORDERINGS:
        sp = gpu.SparseLinearSystemGPU(case.P, case.slots, ordering=o)
        perm = list(gpu.solver.sparse_symbolic(case.P, case.slots, gpu.SparseLinearSystemGPU.ORDERINGS[o])["perm"])
        out.append((f"sparse-{o}", "sparse", sp, perm, True))
        out.append((f"sparse-{o}-multi", "sparse", sp, perm, False))
    return out


def _check(case, ref, rho, label, rc, x, b, c):
    what = f"{case.name} {label}: rho {rho:.3e}"
    assert np.linalg.norm(b - ref.b) <= 1e-13 * np.linalg.norm(ref.b), what + " b"
    assert abs(c - ref.c) <= 1e-13 * abs(ref.c), what + " c"
    if rho >= SOLVES:
        assert rc == GP_OK, what + f" -> {rc}"
        bound = 64 * len(x) * EPS * ref.kappa
        err = np.linalg.norm(x - ref.x) / np.linalg.norm(ref.x)
        assert err <= bound, what + f" |x - x_ref| / |x_ref| = {err:.3e} > {bound:.3e} (kappa {ref.kappa:.3e})"
        bound = 64 * len(x) * EPS * ref.kappa_eq
        err = np.linalg.norm(ref.d * (x - ref.x)) / np.linalg.norm(ref.d * ref.x)
        assert err <= bound, what + f" |D (x - x_ref)| / |D x_ref| = {err:.3e} > {bound:.3e} (equilibrated kappa {ref.kappa_eq:.3e})"
    else:
        assert rho <= INDETERMINATE
        assert rc == GP_ERROR_INDETERMINATE, what + f" -> {rc}, x = {x[:6]}"


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_damped_step_against_the_mpmath_reference(gpu, case):
    import torch

    lib = gpu.load()
    rec_dev = torch.from_numpy(case.records).cuda()
    fs = forms(gpu, case)
    checked, band = 0, []
    for diagonal in (False, True):
        for lam in LAMBDAS:
            ref = reference(case, lam, diagonal)
            for label, kind, obj, order, one in fs:
                rho = ref.rho_for(order)
                if INDETERMINATE < rho < SOLVES:
                    band.append((label, lam, diagonal, rho))
                    continue
                obj.set_one_launch(one)
                for halves in (False, True):
                    rc, x, b, c = _step_call(lib, kind, obj._h, rec_dev, lam, diagonal, case, halves)
                    _check(case, ref, rho, f"{label} lam={lam:g} diag={diagonal} halves={halves}", rc, x, b, c)
                    checked += 1
    # the generator keeps the band between the two margins nearly empty: only the cases whose condition number puts the undamped system there
    assert len(band) <= 2 * len(fs), band
    assert checked >= 8 * len(fs)


def test_the_cases_cover_both_outcomes_in_every_form_family():
    """(host only, no device) the generator is what it claims: singular and solvable systems for the dense one-pose, dense panel and sparse forms, and clipping cases"""
    outcomes = {}
    for case in CASES:
        fam = "one-pose" if case.P == 1 else "multi"
        for lam in (0.0, 1.0):
            rho = reference(case, lam, False).rho["natural"]
            outcomes.setdefault(fam, set()).add("solves" if rho >= SOLVES else ("indeterminate" if rho <= INDETERMINATE else "band"))
    assert {"solves", "indeterminate"} <= outcomes["one-pose"] and {"solves", "indeterminate"} <= outcomes["multi"], outcomes
    assert any(c.max_diag < 1e32 for c in CASES) and any(not c.scalable for c in CASES)
    assert max(6 * c.P for c in CASES) == 72


SCALE_BASE = [c for c in CASES if c.name in ("one-pose-kappa100", "chain3-kappa100", "gauge-free-3", "gauge-prior-3", "plane-axis", "chain12", "isolated")]


@pytest.mark.parametrize("case", SCALE_BASE, ids=[c.name for c in SCALE_BASE])
def test_scaling_the_records_changes_neither_status_nor_step(gpu, case):
    """records and prior x s: the same status and the same x -- to 1e-12 where the damped system is well conditioned, to the backward-error bound 64 n eps kappa_2(A~)
    beyond (lambda x s under lambda I damping; diagonal damping keeps lambda, on cases that do not clip)"""
    import torch

    lib = gpu.load()
    for s in (1e-8, 1e8):
        sc = case.scaled(s)
        dev = [torch.from_numpy(c.records).cuda() for c in (case, sc)]
        for label, kind, obj, order, one in forms(gpu, case):
            obj.set_one_launch(one)
            for diagonal in (False, True):
                if diagonal and not case.scalable:
                    continue
                for lam in (0.0, 1e-5, 1.0):
                    r0 = _step_call(lib, kind, obj._h, dev[0], lam, diagonal, case, False)
                    r1 = _step_call(lib, kind, obj._h, dev[1], lam if diagonal else lam * s, diagonal, sc, False)
                    what = f"{case.name} x{s:g} {label} lam={lam:g} diag={diagonal}"
                    assert r0[0] == r1[0], what + f": status {r0[0]} vs {r1[0]}"
                    if r0[0] == GP_OK:
                        tol = max(1e-12, 64 * 6 * case.P * EPS * reference(case, lam, diagonal).kappa)
                        assert np.linalg.norm(r1[1] - r0[1]) <= tol * np.linalg.norm(r0[1]), what


# ---- B: one step in flight per system ----------------------------------------------------------------------------------------------------------------------------------------
def _lifecycle_records(P, slots, seed):
    rng = np.random.default_rng(seed)
    recs = []
    for st, ss in slots:
        H = _spd(rng, 12, np.logspace(0, -2, 12))
        recs.append(_binary(rng, H) if st >= 0 else _unary(rng, H[6:, 6:]))
    return np.asarray(recs)


@pytest.mark.parametrize("kind,P,one", [("dense", 1, True), ("dense", 1, False), ("dense", 4, True), ("sparse", 4, True), ("sparse", 4, False), ("sparse", 1, True)])
@pytest.mark.parametrize("with_prior", [False, True])
def test_a_second_issue_while_a_step_is_in_flight_is_refused(gpu, kind, P, one, with_prior):
    """issue(rA), issue(rB) before finishing: the second issue fails with GP_ERROR_INVALID_ARGUMENT and finish returns exactly step(rA)'s bits"""
    import torch

    lib = gpu.load()
    slots = [(-1, 0)] + [(i, i + 1) for i in range(P - 1)] + ([(0, P - 1)] if P > 2 else [])
    rA, rB = (torch.from_numpy(_lifecycle_records(P, slots, s)).cuda() for s in (1, 2))
    cls = gpu.DenseLinearSystemGPU if kind == "dense" else gpu.SparseLinearSystemGPU
    sys_, ref = cls(P, slots), cls(P, slots)
    sys_.set_one_launch(one)
    ref.set_one_launch(one)
    n = 6 * P
    priorA = np.linspace(1.0, 2.0, n) if with_prior else None
    priorB = np.linspace(5.0, 3.0, n) if with_prior else None
    want = ref.step(rA, lam=1e-3, prior_diag=priorA)
    issue, finish = getattr(lib, f"gp_{kind}_system_issue_step"), getattr(lib, f"gp_{kind}_system_finish_step")
    pa = priorA.ctypes.data if with_prior else None
    pb = priorB.ctypes.data if with_prior else None
    assert issue(sys_._h, C.c_void_p(rA.data_ptr()), 1e-3, 0, 1e-6, 1e32, pa) == GP_OK
    assert issue(sys_._h, C.c_void_p(rB.data_ptr()), 1e-1, 0, 1e-6, 1e32, pb) == GP_ERROR_INVALID_ARGUMENT
    x, b, c = np.zeros(n), np.zeros(n), np.zeros(1)
    assert finish(sys_._h, x.ctypes.data, b.ctypes.data, c.ctypes.data) == GP_OK
    assert np.array_equal(x, want[0]) and np.array_equal(b, want[1]) and c[0] == want[2]
    assert finish(sys_._h, x.ctypes.data, b.ctypes.data, c.ctypes.data) == GP_ERROR_INVALID_ARGUMENT  # nothing in flight any more
    # ... and the system takes the next step as usual
    got = sys_.step(rB, lam=1e-1, prior_diag=priorB)
    want_b = ref.step(rB, lam=1e-1, prior_diag=priorB)
    assert all(np.array_equal(np.asarray(u), np.asarray(v)) for u, v in zip(got, want_b))
