"""Host-only inputs, metrics and float64 restatements for the tests of the dense symmetric eigensolver
(localmd_amd/csrc/sytrd.hip, sytrd2.hip).  NumPy only; nothing here touches a device (test infrastructure only).

Conventions are the library's: a matrix of eigenvectors E holds eigenvector j in ROW j, eigenvalues ascend."""
import numpy as np

EPS32 = 1.1920929e-07   # the constant of narrow_eigenvalues_kernel

KINDS = ("separated", "repeated", "cluster", "gram_lowrank", "graded", "indefinite", "diagonal", "tridiagonal", "zero_tail",
         "zero", "identity", "tiny", "huge")
LOW_RANK_KINDS = ("gram_lowrank", "zero_tail", "zero")
GAP_SEPARATED_KINDS = ("separated", "indefinite")   # every gap above the refinement's cluster threshold 1e-5 lmax


def _exactly_symmetric(S):
    S = np.asarray(S).astype(np.float32)
    return np.triu(S) + np.triu(S, 1).T


def _separated(rng, n):
    """The random matrix with a well separated spectrum the kernel tests have used from the start (_sym_matrix)."""
    A = rng.standard_normal((n, n)).astype(np.float32)
    S = A @ A.T / np.float32(n) + np.diag(rng.standard_normal(n).astype(np.float32) * 3)
    S = 0.5 * (S + S.T)
    return S.astype(np.float32)


def _conjugated(rng, lam):
    n = lam.size
    q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    return (q * lam) @ q.T


def make_sym(kind, n, seed):
    """float32 (n, n), exactly symmetric after rounding."""
    rng = np.random.default_rng(seed)
    if kind == "separated":
        S = _separated(rng, n)
    elif kind in ("repeated", "cluster"):
        m = min(100, n // 4)
        low = np.ones(m) if kind == "repeated" else 1.0 + 1e-6 * np.arange(m)
        S = _conjugated(rng, np.concatenate([low, np.linspace(2.0, 50.0, n - m)]))
    elif kind == "gram_lowrank":
        r = max(2, n // 15)
        X = rng.standard_normal((n, r)).astype(np.float32) * np.geomspace(1.0, 100.0, r).astype(np.float32)[None, :]
        S = X @ X.T   # fp32 product, as the pipeline forms its Gram matrices
    elif kind == "graded":
        S = _conjugated(rng, np.geomspace(1e-6, 1.0, n))
    elif kind == "indefinite":
        h = n // 2
        half = np.linspace(1.0, 50.0, h)
        S = np.zeros((n, n))
        S[:2 * h, :2 * h] = _conjugated(rng, np.concatenate([-half[::-1], half]))   # n odd: the last row / column stays 0
    elif kind == "diagonal":
        S = np.diag(rng.standard_normal(n))
    elif kind == "tridiagonal":
        e = rng.standard_normal(max(n - 1, 0))
        S = np.diag(rng.standard_normal(n)) + np.diag(e, 1) + np.diag(e, -1)
    elif kind == "zero_tail":
        S = np.zeros((n, n), dtype=np.float32)
        S[:n // 3, :n // 3] = _separated(rng, n // 3)
    elif kind == "zero":
        S = np.zeros((n, n))
    elif kind == "identity":
        S = np.eye(n)
    elif kind == "tiny":
        S = _separated(rng, n) * np.float32(1e-15)
    elif kind == "huge":
        S = _separated(rng, n) * np.float32(1e15)
    else:
        raise ValueError(kind)
    return _exactly_symmetric(S)


def householder_q(A_rows, tau):
    """float64 Q = H_0 H_1 ... H_{n-2} of the reflectors as ssytrd('L') stores them on the column-major view: memory row j of
    A_rows holds v_j = [1 at position j + 1, A_rows[j][j + 2..n)], H_j = I - tau[j] v_j v_j^T."""
    n = A_rows.shape[0]
    Q = np.eye(n)
    for j in range(n - 2, -1, -1):
        v = np.zeros(n)
        v[j + 1] = 1.0
        v[j + 2:] = A_rows[j, j + 2:n]
        Q -= tau[j] * np.outer(v, v @ Q)
    return Q


# ---------------------------------------------------------------------------------------------------------------------
# metrics, all in float64
def _f64(a):
    return np.asarray(a, dtype=np.float64)


def eig_abs_err(w, w_ref):
    return float(np.abs(_f64(w) - _f64(w_ref)).max()) if len(w) else 0.0


def orth_err(E):
    E = _f64(E)
    return float(np.abs(E @ E.T - np.eye(E.shape[0])).max())


def resid(E, S, w):
    E = _f64(E)
    return float(np.abs(E @ _f64(S) - _f64(w)[:, None] * E).max())


def is_ascending(w):
    return bool(np.all(np.diff(_f64(w)) >= 0))


def reference_eigh(S):
    """(w64, V64) of the float32 matrix in float64; eigenvector j is COLUMN j of V64 (numpy.linalg.eigh)."""
    return np.linalg.eigh(_f64(S))


def spectral_groups(w_ref, gap):
    """[(a, b)): index ranges of the ascending reference spectrum that are separated from the rest by more than gap."""
    w_ref = _f64(w_ref)
    cuts = np.nonzero(np.diff(w_ref) > gap)[0] + 1
    edges = [0, *cuts.tolist(), w_ref.size]
    return [(a, b) for a, b in zip(edges[:-1], edges[1:]) if b > a]


def _norm2(M):
    if M.size == 0:
        return 0.0
    if min(M.shape) == 1:
        return float(np.linalg.norm(M))
    return float(np.linalg.norm(M, 2))


def group_sin_theta(E, S, gap, w, ref=None):
    """Per group of the float64 reference spectrum (spectral_groups): (sin, bound) with
         sin   = ||(I - P_ref) E_g^T||_2      the part of the computed vectors of the group outside the reference's invariant
                                              subspace of the same eigenvalues,
         bound = ||S E_g^T - E_g^T L_g||_2 / gap,   L_g = diag(w_g)   (Davis-Kahan: the reference eigenvalues outside the
                                              group are further than gap from the group's).
    E: computed vectors in rows, w: computed (ascending) eigenvalues; row i of E answers reference eigenvalue i."""
    E, S64, w = _f64(E), _f64(S), _f64(w)
    w_ref, V = reference_eigh(S) if ref is None else ref
    C = E @ V                                  # C[i][k] = <computed i, reference k>
    R = E @ S64 - w[:, None] * E               # row i: residual of computed pair i
    out = []
    for a, b in spectral_groups(w_ref, gap):
        outside = np.concatenate([C[a:b, :a], C[a:b, b:]], axis=1)
        out.append((_norm2(outside), _norm2(R[a:b]) / gap if gap > 0 else (0.0 if not R[a:b].any() else np.inf)))
    return out


def floor_null(w64):
    """narrow_eigenvalues_kernel: float64 eigenvalues -> float32, the magnitude of a non-zero one floored at
    eps32 * max |lambda|; as in the kernel, max |lambda| is read from the two ends (ascending order expected)."""
    w64 = _f64(w64)
    if w64.size == 0:
        return w64.astype(np.float32)
    lmax = max(abs(w64[0]), abs(w64[-1]))
    fl = EPS32 * lmax
    small = (w64 != 0.0) & (np.abs(w64) < fl)
    return np.where(small, np.copysign(fl, w64), w64).astype(np.float32)


def refine_reference(S32, w0, E0, steps=2, ordered=True):
    """NumPy restatement of syevd_refine + refine_lambda_kernel + refine_e_kernel + narrow_eigenvalues_kernel of sytrd.hip:
    `steps` Ogita-Aishima steps in float64 on the fp32 solver's output (w0, rows of E0), Rayleigh quotients as eigenvalues.
    ordered: the Rayleigh quotients of the last step are ranked (ties by index) and values and vectors leave in that order,
    as the library does; ordered=False is the routine without that ranking.  Returns (w float32, E float32 with rows)."""
    if steps == 0:
        return np.asarray(w0, dtype=np.float32), np.asarray(E0, dtype=np.float32)
    A = _f64(S32)
    X = _f64(E0).T.copy()                      # columns are vectors
    n = A.shape[0]
    eye = np.eye(n)
    lam = None
    for _ in range(steps):
        AX = A @ X
        Sm = X.T @ AX
        G = X.T @ X
        lam = np.diag(Sm) / np.diag(G)
        lmax = max(abs(lam[0]), abs(lam[-1]))  # the ends of a spectrum assumed ascending
        delta = 1e-5 * lmax
        Rm = eye - G
        dl = lam[None, :] - lam[:, None]       # dl[i][j] = lam_j - lam_i
        far = (np.abs(dl) > delta) & ~np.eye(n, dtype=bool)
        Em = np.where(far, (Sm + lam[None, :] * Rm) / np.where(far, dl, 1.0), 0.5 * Rm)
        X = X + X @ Em
    if ordered:
        order = np.argsort(lam, kind="stable")
        lam, X = lam[order], X[:, order]
    return floor_null(lam), X.T.astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# the bounds the GPU tests hold every route to (tests/test_gpu_kernels.py::_check_syevd_own_path), in one place
def route_bounds(S):
    n = S.shape[0]
    smax = float(np.abs(_f64(S)).max()) if n else 0.0
    return {"eig": 3e-6 * smax * np.sqrt(n), "orth": 5e-5 * np.sqrt(n), "resid": 1e-5 * smax * np.sqrt(n)}
