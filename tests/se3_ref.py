"""Restatement of the SE(3) half of lv_slam_amd/csrc/ndt_math.hpp (= oracle/ndt_oracle.c:416-577: Sophus a621ff2 exp / log / operator*, Eigen 3.3
quaternion <-> matrix, cofactor inverse) over an exchangeable arithmetic, for tests/test_se3_gpu.py and tests/test_se3_cpu.py:

  F64  IEEE double, one rounding per operation in the order the C code writes them, sin / cos / tan / atan from the C library (`math`);
  MP   the same formulas and the same branch rules (the SIGNED `theta < 1e-10` tests, `atan(n / w)` without a |w| special case) in mpmath at 60 digits:
       what the formulas give without rounding, i.e. the value both the oracle and the device are measured against.

Helper module, not a test.  Quaternions are (w, x, y, z) tuples, matrices row-major lists of 9, tangents [upsilon; omega]."""
import functools
import math
import numpy as np
import mpmath

SMALL_EPS = 1e-10
MPCTX = mpmath.mp.clone()
MPCTX.dps = 60


class F64:
    name = "f64"

    @staticmethod
    def num(x):
        return np.float64(x)

    @staticmethod
    def div(a, b):
        with np.errstate(all="ignore"):
            return np.float64(a) / np.float64(b)

    @staticmethod
    def sqrt(x):
        with np.errstate(all="ignore"):
            return np.sqrt(np.float64(x))

    @staticmethod
    def _libm(f, x):
        try:
            return np.float64(f(float(x)))
        except ValueError:                       # (sin / cos / tan of an infinity)
            return np.float64("nan")

    sin = classmethod(lambda c, x: c._libm(math.sin, x))
    cos = classmethod(lambda c, x: c._libm(math.cos, x))
    tan = classmethod(lambda c, x: c._libm(math.tan, x))
    atan = classmethod(lambda c, x: c._libm(math.atan, x))


class MP:
    name = "mp"

    @staticmethod
    def num(x):
        return MPCTX.mpf(float(x))               # every f64 is an exact mpf

    @staticmethod
    def div(a, b):
        if b == 0:                               # IEEE: x / 0 = +-inf, 0 / 0 = NaN (the quaternion of diag(1,-1,-1) has w = +0)
            return MPCTX.nan if (a == 0 or a != a) else (MPCTX.inf if a > 0 else -MPCTX.inf)
        return a / b

    @staticmethod
    def sqrt(x):
        return MPCTX.nan if x < 0 else MPCTX.sqrt(x)

    sin = staticmethod(lambda x: MPCTX.sin(x))
    cos = staticmethod(lambda x: MPCTX.cos(x))
    tan = staticmethod(lambda x: MPCTX.tan(x))
    atan = staticmethod(lambda x: MPCTX.atan(x))


def q_normalized(F, q):
    w, x, y, z = q
    n = F.sqrt(((x * x + y * y) + z * z) + w * w)
    return (F.div(w, n), F.div(x, n), F.div(y, n), F.div(z, n))


def q_branch(m):
    """0: trace > 0; 1 + i: trace <= 0 and diagonal entry i is the one Eigen picks"""
    if m[0] + m[4] + m[8] > 0:
        return 0
    i = 0
    if m[4] > m[0]:
        i = 1
    if m[8] > m[i * 3 + i]:
        i = 2
    return 1 + i


def q_from_matrix(F, m):
    half, one = F.num(0.5), F.num(1.0)
    br = q_branch(m)
    if br == 0:
        t = F.sqrt((m[0] + m[4] + m[8]) + one)
        w = half * t
        t = F.div(half, t)
        return (w, (m[7] - m[5]) * t, (m[2] - m[6]) * t, (m[3] - m[1]) * t)
    i = br - 1
    j = (i + 1) % 3
    k = (j + 1) % 3
    qv = [None] * 3
    t = F.sqrt(m[i * 3 + i] - m[j * 3 + j] - m[k * 3 + k] + one)
    qv[i] = half * t
    t = F.div(half, t)
    w = (m[k * 3 + j] - m[j * 3 + k]) * t
    qv[j] = (m[j * 3 + i] + m[i * 3 + j]) * t
    qv[k] = (m[k * 3 + i] + m[i * 3 + k]) * t
    return (w, qv[0], qv[1], qv[2])


def q_to_matrix(F, q):
    w, x, y, z = q
    two, one = F.num(2.0), F.num(1.0)
    tx, ty, tz = two * x, two * y, two * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return [one - (tyy + tzz), txy - twz, txz + twy,
            txy + twz, one - (txx + tzz), tyz - twx,
            txz - twy, tyz + twx, one - (txx + tyy)]


def q_mul(F, a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return (aw * bw - ax * bx - ay * by - az * bz,
            aw * bx + ax * bw + ay * bz - az * by,
            aw * by + ay * bw + az * bx - ax * bz,
            aw * bz + az * bw + ax * by - ay * bx)


def q_rotate(F, q, v):
    w, x, y, z = q
    uv = [y * v[2] - z * v[1], z * v[0] - x * v[2], x * v[1] - y * v[0]]
    uv = [u + u for u in uv]
    c = [y * uv[2] - z * uv[1], z * uv[0] - x * uv[2], x * uv[1] - y * uv[0]]
    return [(v[i] + w * uv[i]) + c[i] for i in range(3)]


def mat3_mul(F, A, B):
    return [(A[i * 3 + 0] * B[j] + A[i * 3 + 1] * B[3 + j]) + A[i * 3 + 2] * B[6 + j] for i in range(3) for j in range(3)]


def mat3_inverse(F, m):
    def cof(i, j):
        i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
        return m[i1 * 3 + j1] * m[i2 * 3 + j2] - m[i1 * 3 + j2] * m[i2 * 3 + j1]
    c0, c1, c2 = cof(0, 0), cof(1, 0), cof(2, 0)
    det = (c0 * m[0] + c1 * m[3]) + c2 * m[6]
    inv = F.div(F.num(1.0), det)
    return [c0 * inv, c1 * inv, c2 * inv, cof(0, 1) * inv, cof(1, 1) * inv, cof(2, 1) * inv, cof(0, 2) * inv, cof(1, 2) * inv, cof(2, 2) * inv]


def hat3(F, o):
    z = F.num(0.0)
    return [z, -o[2], o[1], o[2], z, -o[0], -o[1], o[0], z]


def so3_exp(F, om):
    """-> (q, theta, small)"""
    theta = F.sqrt((om[0] * om[0] + om[1] * om[1]) + om[2] * om[2])
    half = F.num(0.5) * theta
    real = F.cos(half)
    small = bool(theta < SMALL_EPS)
    if small:
        th2 = theta * theta
        th4 = th2 * th2
        imag = F.num(0.5) - F.num(0.0208333) * th2 + F.num(0.000260417) * th4
    else:
        imag = F.div(F.sin(half), theta)
    return q_normalized(F, (real, imag * om[0], imag * om[1], imag * om[2])), theta, small


def so3_log(F, q):
    """-> (om, theta, n_small)"""
    w, x, y, z = q
    n = F.sqrt((x * x + y * y) + z * z)
    n_small = bool(n < SMALL_EPS)
    two = F.num(2.0)
    if n_small:
        f = F.div(two, w) - F.div(two * (n * n), w * (w * w))
    else:
        f = F.div(two * F.atan(F.div(n, w)), n)
    return [f * x, f * y, f * z], f * n, n_small


def se3_exp(F, p):
    """-> (q, t, small)"""
    q, theta, small = so3_exp(F, p[3:6])
    Om = hat3(F, p[3:6])
    Om2 = mat3_mul(F, Om, Om)
    one, zero = F.num(1.0), F.num(0.0)
    if small:
        V = q_to_matrix(F, q)
    else:
        th2 = theta * theta
        a = F.div(one - F.cos(theta), th2)
        b = F.div(theta - F.sin(theta), th2 * theta)
        V = [((one if i % 4 == 0 else zero) + a * Om[i]) + b * Om2[i] for i in range(9)]
    t = [(V[i * 3 + 0] * p[0] + V[i * 3 + 1] * p[1]) + V[i * 3 + 2] * p[2] for i in range(3)]
    return q, t, small


def se3_log(F, q, t):
    """-> (p, theta, n_small, theta_small)"""
    om, theta, n_small = so3_log(F, q)
    Om = hat3(F, om)
    Om2 = mat3_mul(F, Om, Om)
    one, zero, half = F.num(1.0), F.num(0.0), F.num(0.5)
    theta_small = bool(theta < SMALL_EPS)                     # signed: a large NEGATIVE angle takes the small-angle V^-1 (the reference's Sophus)
    if theta_small:
        c = F.num(1.0 / 12.0)
    else:
        c = F.div(one - F.div(theta, F.num(2.0) * F.tan(F.div(theta, F.num(2.0)))), theta * theta)
    Vi = [((one if i % 4 == 0 else zero) - half * Om[i]) + c * Om2[i] for i in range(9)]
    p = [(Vi[i * 3 + 0] * t[0] + Vi[i * 3 + 1] * t[1]) + Vi[i * 3 + 2] * t[2] for i in range(3)]
    return p + om, theta, n_small, theta_small


def se3_mul(F, qa, ta, qb, tb):
    rt = q_rotate(F, qa, tb)
    return q_normalized(F, q_mul(F, qa, qb)), [ta[i] + rt[i] for i in range(3)]


def vec(F, a):
    return [F.num(x) for x in np.asarray(a, np.float64).ravel()]


def arr(v):
    return np.array([float(x) for x in v], np.float64)


# ---- the evaluations the tests compare, each -> dict of float64 arrays / flags -----------------------------------------------------------

def eval_exp(F, p):
    """se3_exp(p).matrix(): M = [R (9) | t (3)]"""
    q, t, small = se3_exp(F, vec(F, p))
    return dict(q=arr(q), M=np.concatenate([arr(q_to_matrix(F, q)), arr(t)]), small=small)


def eval_log(F, R, t):
    """se3_log(se3_from_Rt(R, t)); "_om": the rotation part before any conversion to f64"""
    m = vec(F, R)
    q = q_normalized(F, q_from_matrix(F, m))
    p, theta, n_small, theta_small = se3_log(F, q, vec(F, t))
    return dict(p=arr(p), theta=float(theta), branch=q_branch(m), n_small=n_small, theta_small=theta_small, _om=p[3:6])


def eval_init(F, G):
    """init_pair_state on an f32 4x4 guess: p = log(guess), R = rotation of exp(p) (what is then rounded to the f32 Rj)"""
    G = np.asarray(G, np.float32).astype(np.float64)
    r = eval_log(F, G[:3, :3].ravel(), G[:3, 3])
    q, _, _ = so3_exp(F, r["_om"])
    r["R"] = arr(q_to_matrix(F, q))
    return r


def eval_compose(F, dp, p):
    """se3_log(se3_mul(se3_exp(dp), se3_exp(p))) and exp(dp).matrix()"""
    qd, td, _ = se3_exp(F, vec(F, dp))
    qp, tp, _ = se3_exp(F, vec(F, p))
    q, t = se3_mul(F, qd, td, qp, tp)
    pn, theta, n_small, theta_small = se3_log(F, q, t)
    return dict(p=arr(pn), w=float(q[0]), theta=float(theta), theta_small=theta_small, inc=np.concatenate([arr(q_to_matrix(F, qd)), arr(td)]))


def rotation_mp(theta, axis):
    """Rodrigues' rotation matrix of angle theta (an f64) about `axis` (normalised at 60 digits), rounded once to f64; row-major 9"""
    a = [MPCTX.mpf(float(x)) for x in axis]
    n = MPCTX.sqrt(sum(x * x for x in a))
    a = [x / n for x in a]
    th = MPCTX.mpf(float(theta))
    c, s = MPCTX.cos(th), MPCTX.sin(th)
    K = [[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]]
    R = [[(c if i == j else 0) + (1 - c) * a[i] * a[j] + s * K[i][j] for j in range(3)] for i in range(3)]
    return np.array([float(R[i][j]) for i in range(3) for j in range(3)], np.float64) + 0.0


# ---- the records of tests/hip/se3_check (REC_IN doubles in, REC_OUT doubles out per record) ----------------------------------------------
REC_IN, REC_OUT = 32, 72
PI = math.pi
TH_SMALL = [0.0, 1e-12, 9.9e-11, 1e-10, 1.1e-10, 3e-10, 1e-9, 1e-8, 1e-7, 1e-6, 1e-5, 1e-3]      # around the 1e-10 threshold of exp / log
TH_LARGE = [PI / 2, 2 * PI / 3 - 1e-9, 2 * PI / 3 + 1e-9, 2.5, PI - 1e-3, PI - 1e-8, PI, PI + 1e-8, 4.0, 2 * PI - 1e-6, 7.0]   # trace <= 0, w -> 0, w < 0
MAGS = [0.0, 1e-3, 1.0, 1e3, 1e5]                                                                # translation magnitudes


def theta_class(th):
    """small: the series branch; cancel: (1 - cos theta) / theta^2 loses digits on any libm (theta just above 1e-10 up to 1e-5); mid; large"""
    return "small" if th < 1e-10 else "cancel" if th <= 1e-5 else "mid" if th < 1.0 else "large"


def _unit(rng, n=3):
    v = rng.normal(size=n)
    return v / np.linalg.norm(v)


def special_matrices(rng):
    """(name, row-major 9) for q_from_matrix / init_pair_state: every branch, the half turns, a tie on the diagonal; each also rounded to f32"""
    out = [("trace_pos", rotation_mp(1.0, _unit(rng)))]
    for i in range(3):
        ax = 0.15 * _unit(rng)
        ax[i] = 1.0
        out.append((f"diag{i}_largest", rotation_mp(2.8, ax)))
    out += [("half_turn_x", np.diag([1.0, -1.0, -1.0]).ravel()), ("half_turn_y", np.diag([-1.0, 1.0, -1.0]).ravel()), ("half_turn_z", np.diag([-1.0, -1.0, 1.0]).ravel())]
    tie = rotation_mp(2.8, [1.0, 1.0, 0.3])
    tie[4] = tie[0]                                                # m[4] == m[0] exactly: `m[4] > m[0]` is false, i stays 0
    out.append(("tie_m4_m0", tie))
    tie2 = rotation_mp(2.9, [0.3, 1.0, 1.0])
    tie2[8] = tie2[4]                                              # m[8] == m[4] > m[0]: i = 1 stays
    out.append(("tie_m8_m4", tie2))
    return out + [(n + "_f32", m.astype(np.float32).astype(np.float64)) for n, m in out]


@functools.lru_cache(maxsize=1)
def cases():
    """The list of records: dicts with kind, cls, rec (REC_IN doubles) and the inputs by name."""
    rng = np.random.default_rng(20261018)
    axes = [np.array([1.0, 0, 0]), np.array([0, 1.0, 0]), np.array([0, 0, 1.0]), np.ones(3) / np.sqrt(3.0), _unit(rng), _unit(rng)]
    thetas = TH_SMALL + TH_LARGE
    spec = special_matrices(rng)
    C = []

    def add(kind, cls, payload, **kw):
        rec = np.zeros(REC_IN)
        rec[0] = kind
        rec[1:1 + len(payload)] = payload
        C.append(dict(kind=kind, cls=cls, rec=rec, **kw))

    # kind 1: se3_exp / pose_to_f32
    for it, th in enumerate(thetas):
        for ia, ax in enumerate(axes):
            p = np.concatenate([MAGS[(it + ia) % 5] * _unit(rng), th * ax])
            add(1, theta_class(th), p, p=p)
    # kind 2: se3_log(se3_from_Rt);  kind 0: the quaternion / matrix helpers on the same matrices
    mats = [(theta_class(th), rotation_mp(th, ax), (it + ia + 2) % 5) for it, th in enumerate(thetas) for ia, ax in enumerate(axes)]
    mats += [("matrix", m, k % 5) for k, (_, m) in enumerate(spec)]
    for cls, R, im in mats:
        t = MAGS[im] * _unit(rng)
        add(2, cls, np.concatenate([R, t]), R=R, t=t)
    general = [rotation_mp(rng.uniform(0, 3.0), _unit(rng)) + 0.1 * rng.normal(size=9) for _ in range(6)]
    for cls, R, im in mats + [("general", m, k % 5) for k, m in enumerate(general)]:
        q2 = rng.normal(size=4) * 10.0 ** rng.integers(-3, 4)
        v, t1, t2 = MAGS[im] * _unit(rng), MAGS[(im + 1) % 5] * _unit(rng), MAGS[(im + 3) % 5] * _unit(rng)
        add(0, cls, np.concatenate([R, q2, v, t1, t2]), m=R, q2=q2, v=v, t1=t1, t2=t2)
    # kind 3: init_pair_state on the f32 guess
    for cls, R, im in mats:
        G = np.eye(4, dtype=np.float32)
        G[:3, :3] = R.reshape(3, 3).astype(np.float32)
        G[:3, 3] = (MAGS[(im + 1) % 5] * _unit(rng)).astype(np.float32)
        add(3, cls, G.ravel(order="F").astype(np.float64), G=G)
    # kind 4: newton_rebase(p, dir, a_t)
    for it, th in enumerate(thetas):
        for ik, a_t in enumerate((1e-6, 1e-2, 0.5)):
            p = np.concatenate([MAGS[(it + ik) % 5] * _unit(rng), th * axes[(it + ik) % 6]])
            d = _unit(rng, 6)
            add(4, theta_class(th), np.concatenate([p, d, [a_t]]), p=p, dir=d, a_t=a_t)
    for ax in (axes[2], axes[4]):                                  # the product turns past pi: its quaternion has w < 0
        for a_t in (1e-2, 0.5):
            p = np.concatenate([_unit(rng), (PI - 1e-3) * ax])
            d = np.concatenate([0.3 * _unit(rng), ax])
            d /= np.linalg.norm(d)
            add(4, "large", np.concatenate([p, d, [a_t]]), p=p, dir=d, a_t=a_t)
    # NaN in, NaN out, and the program ends
    nan = float("nan")
    p = np.array([0.5, -0.2, 0.1, 0.3, nan, -0.4])
    add(1, "nan", p, p=p)
    d = _unit(rng, 6)
    add(4, "nan", np.concatenate([p, d, [0.1]]), p=p, dir=d, a_t=0.1)
    for pos in ((0, 1), (1, 3)):
        G = np.eye(4, dtype=np.float32)
        G[:3, :3] = rotation_mp(0.7, axes[4]).reshape(3, 3).astype(np.float32)
        G[:3, 3] = (0.5, 1.0, -2.0)
        G[pos] = nan
        add(3, "nan", G.ravel(order="F").astype(np.float64), G=G)
    return C


def write_records(path):
    np.ascontiguousarray(np.stack([c["rec"] for c in cases()])).tofile(path)


@functools.lru_cache(maxsize=1)
def references():
    """Per record of kinds 1..4: (oracle, f64 restatement, mpmath) evaluations; kind 0: the f64 restatement.  Computed once per session."""
    from oracle import oracle_py as O
    out = []
    for c in cases():
        k = c["kind"]
        if k == 0:
            F = F64
            m = vec(F, c["m"])
            qf = q_from_matrix(F, m)
            qn = q_normalized(F, qf)
            q2n = q_normalized(F, tuple(vec(F, c["q2"])))
            qm, tm = se3_mul(F, qn, vec(F, c["t1"]), q2n, vec(F, c["t2"]))
            out.append(dict(f64=np.concatenate([arr(qf), [float(q_branch(m))], arr(qn), arr(q_to_matrix(F, qn)), arr(q2n), arr(q_mul(F, qn, q2n)),
                                                arr(q_rotate(F, qn, vec(F, c["v"]))), arr(qm), arr(tm), arr(mat3_inverse(F, m))])))
            continue
        nan = c["cls"] == "nan"
        if k == 1:
            M = O.se3_exp(c["p"])
            r = dict(ora=np.concatenate([M[:3, :3].ravel(), M[:3, 3]]), f64=eval_exp(F64, c["p"]), mp=None if nan else eval_exp(MP, c["p"]))
        elif k == 2:
            M = np.eye(4)
            M[:3, :3] = c["R"].reshape(3, 3)
            M[:3, 3] = c["t"]
            r = dict(ora=O.se3_log(M), f64=eval_log(F64, c["R"], c["t"]), mp=None if nan else eval_log(MP, c["R"], c["t"]))
        elif k == 3:
            po = O.se3_log(c["G"].astype(np.float64))
            r = dict(ora=po, ora_R=O.se3_exp(po)[:3, :3].ravel(), f64=eval_init(F64, c["G"]), mp=None if nan else eval_init(MP, c["G"]))
        else:
            dp = c["dir"] * c["a_t"]
            r = dict(ora=O.se3_compose_log(dp, c["p"]), f64=eval_compose(F64, dp, c["p"]), mp=None if nan else eval_compose(MP, dp, c["p"]))
        out.append(r)
    return out


def scaled_err(got, want):
    """(largest |got - want| / max(1, largest |want|), one ulp of want's largest component on the same scale)"""
    want = np.asarray(want, np.float64)
    big = float(np.abs(want).max())
    scale = max(1.0, big)
    return float(np.abs(np.asarray(got, np.float64) - want).max()) / scale, float(np.spacing(big)) / scale
