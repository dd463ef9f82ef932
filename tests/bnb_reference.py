"""Exact per-node reference of fit(BnB): the relaxed lower bound of a node (BnB.jl:69-92) and its branch group (BnB.jl:42-57,107,117).
TEST INFRASTRUCTURE ONLY (imported by tests; not a conftest.py, not collected).

A node is (pat, free) over the K' = K + 1 groups of the homogeneous problem (bit K is the intercept's group): group k is branched iff
bit k of `free` is clear, and then constrains its members to alpha >= 0 (bit k of `pat` set) or <= 0.  Σ accumulates the constraints of
every branched group (BnB.jl:120-121), so a variable with both kinds is fixed at 0 (BnB.jl:74-79: both of its columns are zeroed) and a
variable with none is free.

The reference solves that relaxation without the literal [Xp Xm] split (2 M' columns): the columns fixed at 0 are dropped, the <= 0
columns flipped, the free columns projected out (orthonormal basis of their range from an SVD, so duplicate and null columns are
harmless) and the sign-constrained rest goes to Lawson-Hanson NNLS (oracle.nnls) on the QR-compressed problem (oracle.compress, M'+1
rows, the same residual norm for every w).  The solution is then CERTIFIED: least squares is solved again on the support found (free
variables included), the primal signs and the dual signs (gradient of the constrained variables at zero) are checked with a margin,
and the objective is evaluated on the regularised data in long double.  A node that fails the check is reported (certified = False);
nothing is guessed.  nu_k = (sum of w+)(sum of |w-|) over group k from the certified w; branch = first maximal index, -1 when every
nu_k is 0 (the relaxed solution is feasible, BnB.jl:109-115).
"""
import numpy as np

U = 2.0 ** -53                         # unit round-off of fp64
PRIMAL_MARGIN = 1e-10                  # a support variable may sit this far (in units of ||z|| / ||x_j||) on the wrong side of 0
DUAL_MARGIN = 1e-10                    # KKT gradient margin, in units of ||x_j|| ||z||


def ld_data_objective(X, y, w, t, block=32):
    """||y - X w - t|| in long double, X in column blocks (memory stays at one block of long doubles)."""
    r = y.astype(np.longdouble) - np.longdouble(t)
    for j0 in range(0, X.shape[1], block):
        j1 = min(X.shape[1], j0 + block)
        nz = np.flatnonzero(w[j0:j1])
        if len(nz):
            r -= X[:, j0 + nz].astype(np.longdouble) @ w[j0:j1][nz].astype(np.longdouble)
    return float(np.sqrt(np.dot(r, r)))


def node_codes(Po, pat, free):
    """Per-variable constraint of node (pat, free) over the M' homogeneous variables: 1 (>= 0), -1 (<= 0), 2 (free), 0 (fixed at 0:
    Σ holds both i and -i)."""
    Mp, Kp = Po.shape
    pat, free = int(pat), int(free)
    posg = [k for k in range(Kp) if not (free >> k) & 1 and (pat >> k) & 1]
    negg = [k for k in range(Kp) if not (free >> k) & 1 and not (pat >> k) & 1]
    pos = Po[:, posg].any(axis=1) if posg else np.zeros(Mp, dtype=bool)
    neg = Po[:, negg].any(axis=1) if negg else np.zeros(Mp, dtype=bool)
    codes = np.full(Mp, 2, dtype=np.int8)
    codes[pos & ~neg] = 1
    codes[neg & ~pos] = -1
    codes[pos & neg] = 0
    return codes


def nu_groups(w, Po):
    """nu_k = (sum of the positive w)(sum of the |negative w|) over the members of group k"""
    wp = np.clip(w, 0.0, None)
    wn = np.clip(-w, 0.0, None)
    return (Po.T.astype(np.float64) @ wp) * (Po.T.astype(np.float64) @ wn)


def nu_pairwise(w, Po):
    """BnB.jl:42-57 as written: nu_k = sum over pairs i < j of group k of max(0, -w_i w_j) (small cases only)"""
    Kp = Po.shape[1]
    out = np.zeros(Kp)
    for k in range(Kp):
        m = np.flatnonzero(Po[:, k])
        out[k] = sum(max(0.0, -w[i] * w[j]) for a, i in enumerate(m) for j in m[a + 1:])
    return out


def first_argmax(nu):
    """(branch, gap): first maximal index (-1 when every nu_k is 0) and the gap between the two largest values"""
    kb = int(np.argmax(nu))
    s = np.sort(nu)[::-1]
    gap = float(s[0] - s[1]) if len(s) > 1 else float(s[0])
    return (kb if nu[kb] > 0.0 else -1), gap


def _range_basis(A):
    """orthonormal basis of range(A) (rank-revealing: duplicate and null columns drop out)"""
    if A.shape[1] == 0:
        return np.zeros((A.shape[0], 0))
    Uu, sv, _ = np.linalg.svd(A, full_matrices=False)
    if not len(sv) or sv[0] == 0.0:
        return np.zeros((A.shape[0], 0))
    r = int(np.sum(sv > sv[0] * max(A.shape) * np.finfo(np.float64).eps))
    return Uu[:, :r]


class NodeReference:
    """The relaxation of every node of one problem: homogeneous + regularised data, compressed once."""

    def __init__(self, X, y, P, eta=0.0):
        from oracle import oracle as O
        self.O = O
        X = np.asfortranarray(X, dtype=np.float64)
        P = np.asfortranarray(P, dtype=np.int64)
        Xo, Po = O.homogeneous(X, P)
        self.Xn, self.yn = O.regularize(Xo, np.ascontiguousarray(y, dtype=np.float64), Po, eta)
        self.Po = Po
        self.Mp, self.Kp = Po.shape
        self.R, self.z = O.compress(self.Xn, self.yn)
        self.cn = np.linalg.norm(self.R, axis=0)                       # ||x_j|| on the regularised data
        self.zn = float(np.linalg.norm(self.z))
        self.yy = float(np.dot(self.yn.astype(np.longdouble), self.yn.astype(np.longdouble)))

    # ---- the relaxation ------------------------------------------------------------------------------------------------------
    def solve(self, codes):
        """(w, certified): the relaxed optimum for per-variable codes (projected form + NNLS, then the certification)"""
        R, z = self.R, self.z
        F = np.flatnonzero(codes == 2)
        Cc = np.flatnonzero((codes == 1) | (codes == -1))
        s = codes[Cc].astype(np.float64)
        Q = _range_basis(R[:, F])
        AC = R[:, Cc] * s
        x = np.zeros(len(Cc))
        if len(Cc):
            ACp = AC - Q @ (Q.T @ AC)
            # a constrained column inside the range of the free ones (a duplicate of a free column) adds nothing: its projection is
            # round-off, which NNLS would otherwise take at a huge weight
            ACp[:, np.linalg.norm(ACp, axis=0) <= 1e-9 * np.linalg.norm(AC, axis=0)] = 0.0
            x = self.O.nnls(ACp, z - Q @ (Q.T @ z))[0]
        S = Cc[x > 0.0]
        cols = np.concatenate([F, S]).astype(np.int64)
        w = np.zeros(self.Mp)
        if len(cols):
            w[cols] = np.linalg.lstsq(R[:, cols], z, rcond=None)[0]
        w, ok = self.certify(codes, w)
        if ok or not len(F) + len(S):
            return w, ok
        # dependent columns on the support (a duplicate pair with opposite constraints): the minimum-norm re-solve may split the pair
        # across a sign; NNLS's own point, free variables by least squares on its residual, is then the candidate
        w = np.zeros(self.Mp)
        w[Cc] = s * x
        if len(F):
            w[F] = np.linalg.lstsq(R[:, F], z - AC @ x, rcond=None)[0]
        return self.certify(codes, w)

    def certify(self, codes, w):
        """primal signs on the support, dual signs off it, stationarity of the free variables — each with a margin"""
        w = w.copy()
        c = self.cn
        zn = self.zn if self.zn > 0.0 else 1.0
        ok = True
        con = (codes == 1) | (codes == -1)
        sw = np.where(con, codes * w, 0.0)
        bad = con & (sw < -PRIMAL_MARGIN * zn / np.where(c > 0.0, c, 1.0))
        ok &= not bad.any()
        w[con & (sw < 0.0)] = 0.0                                      # within the margin: onto the constraint
        w[codes == 0] = 0.0
        g = self.R.T @ (self.z - self.R @ w)                           # minus the gradient of 1/2 ||R w - z||^2
        tol = DUAL_MARGIN * c * zn
        act = (codes == 2) | (con & (w != 0.0))
        ok &= bool(np.all(np.abs(g[act]) <= tol[act]))
        ina = con & (w == 0.0)
        ok &= bool(np.all(codes[ina] * g[ina] <= tol[ina]))
        return w, bool(ok)

    def node(self, pat, free):
        codes = node_codes(self.Po, pat, free)
        w, cert = self.solve(codes)
        lb = ld_data_objective(self.Xn, self.yn, w, 0.0)
        nu = nu_groups(w, self.Po)
        branch, gap = first_argmax(nu)
        return dict(lb=lb, branch=branch, w=w, nu=nu, gap=gap, certified=cert, codes=codes)

    def nodes(self, pats, frees):
        rs = [self.node(p, f) for p, f in zip(np.asarray(pats).tolist(), np.asarray(frees).tolist())]
        return dict(lb=np.array([r["lb"] for r in rs]), branch=np.array([r["branch"] for r in rs], dtype=np.int32),
                    w=np.array([r["w"] for r in rs]).reshape(len(rs), self.Mp), nu=np.array([r["nu"] for r in rs]).reshape(len(rs), self.Kp),
                    gap=np.array([r["gap"] for r in rs]), certified=np.array([r["certified"] for r in rs], dtype=bool),
                    codes=np.array([r["codes"] for r in rs], dtype=np.int8).reshape(len(rs), self.Mp))

    # ---- the other forms of the same relaxation (self-tests) ---------------------------------------------------------------
    def literal_split(self, pat, free):
        """BnB.jl:69-92 as written: NNLS on [Xp Xm] of the regularised data, Xp[:, negConstr] = 0, Xm[:, posConstr] = 0"""
        codes = node_codes(self.Po, pat, free)
        Xp = self.Xn.copy()
        Xm = -self.Xn
        Xp[:, (codes == -1) | (codes == 0)] = 0.0
        Xm[:, (codes == 1) | (codes == 0)] = 0.0
        x, rn, mode, _ = self.O.nnls(np.column_stack([Xp, Xm]), self.yn)
        return rn, x[:self.Mp] - x[self.Mp:]

    def brute_force(self, pat, free):
        """min over every orthant of the free variables of NNLS with all of them sign-constrained (<= 8 free variables)"""
        codes = node_codes(self.Po, pat, free)
        F = np.flatnonzero(codes == 2)
        assert len(F) <= 8
        best = np.inf
        for o in range(1 << len(F)):
            cc = codes.copy()
            cc[F] = [1 if (o >> i) & 1 else -1 for i in range(len(F))]
            keep = np.flatnonzero(cc != 0)
            A = self.R[:, keep] * cc[keep].astype(np.float64)
            rn = self.O.nnls(A, self.z)[1] if len(keep) else float(np.linalg.norm(self.z))
            best = min(best, rn)
        return best


def bnb_node_reference(X, y, P, eta, pats, frees):
    """Per node (pat, free): lb, branch, the certified w (M' homogeneous variables), nu (K' groups), the gap between the two largest nu
    and whether the solution was certified."""
    return NodeReference(X, y, P, eta).nodes(pats, frees)
