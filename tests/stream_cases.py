"""Op-level cases of the tensor streams — K10 (fill_rank = build_V, residual_sq = ||V - [[W]]||^2 and ||V||^2), the
generators (fill_uniform, fill_laplacian, add_uniform_noise, uniform_sumsq) and the layout and shard ops (pad_layout,
unpack_shards, upload_shard / download_shard, the plain krp) — with their one checker (tests/test_gpu_streams.py on the
HIP kernels, tests/test_streams_hostsim.py on the host stand-in, both through tests/opshim), in the style of
tests/update_cases.py; buffers, image checker, route checker and storage rounding are those of
tests/contraction_cases.py.

A case is a plain dict: the op, its arguments, `route` (regular expressions each of which must match a tag of the
calls' route log) and `why`. The K10 tags are computed from the launchers' formulas restated below (rank_plan, the
k_split call of rank_split, the kch rule of rank_stream), never copied from a run. `dev=True` marks a case whose chunk
count rests on the CU count (rank.mfma / rank.split with more than one k-chunk): sized for 256 CUs, skipped with a
message elsewhere.

Per case: every input is followed by 4 KiB of NaN, every output lies between two 4 KiB NaN guards; after the calls
every byte outside the results is unchanged and no result is NaN. Every case runs TWICE on fresh buffers and the two
sets of output images must be equal bit for bit (the partial sums and k_sum_partials have fixed orders). References
are numpy in long double; u = 2^-53. u_dt is the unit roundoff of the storage type: 0 for f64, 2^-24 for f32 and, for
bf16, what csrc/bf16.h implements — fp64 -> fp32 -> bf16 (8 significant bits), both to nearest even, so
      |bf16(x) - x| <= 2^-8 |fl32(x)| + 2^-24 |x| <= (2^-8 + 2^-24 + 2^-32) |x|      =: u_bf16.

Bars, all derived, none tuned. With a = (|Q||P|)[m, k] and m the long-double model:
* fill_rank:        |V - m| <= (R + 1) u a + u_dt (|m| + (R + 1) u a);
* residual_sq with a model: e = V_stored - m, delta = (R + 2) u a + u |e| (an MFMA or fma chain in any order, the REM
  ranks subtracted one by one), n = M K; the result must lie in
      [ sum max(|e| - delta, 0)^2 (1 - (n + 2) u),  sum (|e| + delta)^2 (1 + (n + 2) u) ];
  err/bar is reported as the distance from sum e^2 in units of the distance of the nearer end;
* residual_sq with Q null and uniform_sumsq: (n + 2) u relative to the long-double sum of squares (of V as stored,
  resp. of x = lo + (hi - lo) u01 evaluated exactly; the <= 2 u (|lo| + |hi - lo| u01) of the device's own x moves
  the sum by less than 20 u for the three ranges used, far inside (n + 2) u at the n >= 3913 of every case);
* fill_uniform: splitmix64 / u01 restated in numpy uint64; x carries at most two roundings (fewer under fma),
  E = 2 u (|lo| + |hi - lo| u01), then the one storage rounding: E + u_dt (|x| + E);
* add_uniform_noise: two more roundings on |V| + |alpha x|: E_n = |alpha| E + 2 u (|V| + |alpha x|), then the storage
  rounding E_n + u_dt (|V + alpha x| + E_n);
* fill_laplacian, pad_layout (pad elements zero), unpack_shards (the NaN filler between the staged shards must not
  appear), upload_shard (== _stored(x, dt)) and download_shard (the shard's rows in a NaN-filled host tensor, every
  other row still NaN): exact, compared as bytes;
* krp: (nf - 1) u |ref|.

Value classes of K10's residual: `far` V independent of the factors, `at` V the stored model of the same factors,
`spike` = `at` plus one entry of 1024 whose position moves over the cases among the last row of the last tile, the
last column of the last partial block, row 0 / column 0 and the first column of the second chunk.

Not covered, because no shape of test size reaches them (nothing forces them):
* the rem = 0 fallback of rank_plan when a chunk's REM share of P exceeds 48 KiB: needs per > 384 column blocks a
  chunk, i.e. K >= 16 * 385 * 4096 (25 M columns) at one row tile on 256 CUs, or 4096 row tiles (M = 2^20 fp32 rows)
  by K >= 6160 — 25 GB of tensor;
* nchunk > 65535: a launcher never asks for more than 16 chunks per CU, so this needs more than 4095 CUs;
* the int-range refusals: more than 2^31 - 1 column blocks (K > 3.4e10) or row tiles (M > 2^31 * 64 VEC).
"""
import numpy as np

import contraction_cases as CC
from contraction_cases import GUARD, VEC, _stored, check_image, check_route
from opshim_util import BF16, F32, F64

U = 2.0 ** -53
LD = np.longdouble
TINY = np.finfo(np.float64).tiny
DT = {"f32": F32, "f64": F64, "bf16": BF16}
NPT = {"f32": np.dtype(np.float32), "f64": np.dtype(np.float64), "bf16": np.dtype(np.uint16)}
UDT = {"f64": 0.0, "f32": 2.0 ** -24, "bf16": 2.0 ** -8 + 2.0 ** -24 + 2.0 ** -32}
WORST = {}  # family -> largest err / bar seen (profiles/stream_ops_bars.md)
SPIKE = 1024.0


# ------------------------------------------------------------------------------------------ the launchers' formulas
def k_split(n, want, min_per=1, align=1):
    """hip_ops.hip: k_split -> (nsplit, per)"""
    want = max(want, 1)
    per = max(-(-n // want), min_per)
    per = -(-per // align) * align
    return -(-n // per), per


def rank_plan(mode, dt, M, K, R, aligned=True, ncu=256):
    """hip_ops.hip: rank_plan and the instantiation rank_mfma picks -> dict, or None where the shape is refused"""
    if dt == "bf16":
        return None
    v = VEC[dt]
    if R > 32 or M % v or M < v or not aligned or K < 1:
        return None
    nkb, tiles = -(-K // 16), -(-M // (64 * v))
    chunks, per = k_split(nkb, min(nkb, (ncu * 16 + tiles - 1) // tiles), min(nkb, 8))
    rem = R % 4 if (mode in (1, 3) and 4 < R <= 17 and (R % 4 == 1 or (R % 4 == 2 and R <= 10))) else 0
    if 8 * per * 16 * rem > 48 * 1024:
        rem = 0
    RB = 1 if mode == 2 else (R - rem + 3) // 4
    if mode == 1 and rem:
        maxrb = 2 if RB <= 2 else 4
    else:
        maxrb, rem = (3 if RB <= 3 else 4 if RB <= 4 else 8), 0
    return dict(maxrb=maxrb, rem=rem, tiles=tiles, chunks=chunks, per=per)


def split_plan(mode, dt, M, K, R, aligned=True, ncu=256):
    """hip_ops.hip: rank_split"""
    if dt == "bf16" or mode == 2:
        return None
    v = VEC[dt]
    if R <= 32 or R > 256 or M % v or M < v or not aligned or K < 1:
        return None
    RB, nkb, tiles = (R + 3) // 4, -(-K // 16), -(-M // (16 * v))
    chunks, per = k_split(nkb, min(nkb, (ncu * 8 + tiles - 1) // tiles), min(nkb, 8))
    rbw = (RB + 3) // 4
    return dict(maxrbw=4 if rbw <= 4 else 8 if rbw <= 8 else 16, tiles=tiles, chunks=chunks, per=per)


def stream_plan(K, R):
    """hip_ops.hip: rank_stream's own launch"""
    kch = 32
    while -(-K // kch) > 65535:
        kch *= 2
    return dict(rb=0 if R > 64 else 16 if R <= 16 else 32 if R <= 32 else 64, kch=kch)


def rank_route(mode, dt, M, K, R, aligned=True):
    """-> (launcher, the tag's regular expression, dev)"""
    Rt = 0 if mode == 2 else R
    p = rank_plan(mode, dt, M, K, Rt, aligned)
    if p:
        return ("mfma", rf"rank\.mfma mode={mode} dt={dt} R={Rt} maxrb={p['maxrb']} rem={p['rem']} "
                        rf"tiles={p['tiles']} chunks={p['chunks']} per={p['per']}", p["chunks"] > 1)
    p = split_plan(mode, dt, M, K, Rt, aligned)
    if p:
        return ("split", rf"rank\.split mode={mode} dt={dt} R={Rt} maxrbw={p['maxrbw']} tiles={p['tiles']} "
                         rf"chunks={p['chunks']} per={p['per']}", p["chunks"] > 1)
    p = stream_plan(K, Rt)
    return "stream", rf"rank\.stream mode={mode} dt={dt} R={Rt} rb={p['rb']} kch={p['kch']}", False


def tag_family(tag):
    """`rank.mfma mode=1 dt=f32 R=13 maxrb=4 rem=1 tiles=2 ...` -> `rank.mfma mode=1 dt=f32 maxrb=4 rem=1`: the
    kernel instantiation"""
    f = dict(kv.split("=") for kv in tag.split(" ")[1:])
    keys = {"rank.mfma": ("mode", "dt", "maxrb", "rem"), "rank.split": ("mode", "dt", "maxrbw"),
            "rank.stream": ("mode", "dt", "rb")}[tag.split(" ")[0]]
    return tag.split(" ")[0] + "".join(f" {k}={f[k]}" for k in keys)


def _expected_tags():
    """every instantiation the three launchers can log, from the formulas above over every rank they accept"""
    out = set()
    for dt in ("f32", "f64"):
        v = VEC[dt]
        for mode in (0, 1, 2):
            for R in ((0,) if mode == 2 else range(1, 33)):
                p = rank_plan(mode, dt, v, 16, R)
                out.add(f"rank.mfma mode={mode} dt={dt} maxrb={p['maxrb']} rem={p['rem']}")
        for mode in (0, 1):
            for R in range(33, 257):
                out.add(f"rank.split mode={mode} dt={dt} maxrbw={split_plan(mode, dt, v, 16, R)['maxrbw']}")
    for dt in ("f32", "f64", "bf16"):
        for mode in (0, 1, 2):
            for R in ((0,) if mode == 2 else range(1, 300)):
                out.add(f"rank.stream mode={mode} dt={dt} rb={stream_plan(16, R)['rb']}")
    return sorted(out)


EXPECTED_TAGS = _expected_tags()


# ------------------------------------------------------------------------------------------ helpers
def vals(rng, cls, shape):
    x = rng.random(shape)
    return 0.5 + 0.5 * x if cls == "pos" else 2.0 * x - 1.0


def decode(a, dt):
    """storage elements -> their exact fp64 values"""
    a = np.asarray(a)
    if dt == "bf16":
        return (a.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    return a.astype(np.float64)


def encode(x, dt):
    """fp64 values -> storage elements, rounded as the tensor stores them"""
    return np.ascontiguousarray(_stored(np.asarray(x, dtype=np.float64), dt)[1]).astype(NPT[dt], copy=False)


def _worst(fam, ratio):
    WORST[fam] = max(WORST.get(fam, 0.0), float(ratio))


class Within:
    """an expectation |got - ref| <= bar, elementwise (bar 0: exact)"""

    def __init__(self, ref, bar):
        self.ref, self.bar = np.asarray(ref, dtype=LD), np.broadcast_to(np.asarray(bar, dtype=LD), np.shape(ref))

    def check(self, c, what, got, log=None):
        got = np.asarray(got, dtype=np.float64).reshape(self.ref.shape)
        err = np.abs(got.astype(LD) - self.ref)
        ratio = float(np.max(np.where(err == 0, LD(0), err / np.maximum(self.bar, TINY)))) if err.size else 0.0
        _worst(c["family"], ratio)
        if log is not None:
            log.append(f"{c['name']} {what}: max err/bar {ratio:.3g}")
        bad = np.argwhere(err > self.bar)
        assert bad.size == 0, (f"{c['name']} {what}: {len(bad)} elements over the bar, first at {tuple(bad[0])}: err "
                               f"{float(err[tuple(bad[0])]):.3e} bar {float(self.bar[tuple(bad[0])]):.3e}")

    def moved(self, got, e, k=4.0):
        """got[e] moved by k bars (exact expectations: by one)"""
        return got[e] + (k * float(self.bar.reshape(-1)[e]) or 1.0)


class Interval:
    """an expectation lo <= got <= hi around `mid`"""

    def __init__(self, lo, mid, hi):
        self.lo, self.mid, self.hi = LD(lo), LD(mid), LD(hi)
        assert self.lo <= self.mid <= self.hi

    def check(self, c, what, got, log=None):
        g = LD(np.asarray(got, dtype=np.float64).reshape(-1)[0])
        d = g - self.mid
        ratio = float(d / max(self.hi - self.mid, LD(TINY)) if d >= 0 else -d / max(self.mid - self.lo, LD(TINY)))
        _worst(c["family"], ratio)
        if log is not None:
            wide = float((self.hi - self.lo) / max(self.mid, LD(TINY)))
            log.append(f"{c['name']} {what}: err/bar {ratio:.3g} (interval {wide:.3g} of the sum wide)")
        assert self.lo <= g <= self.hi, (f"{c['name']} {what}: {float(g):.17g} outside [{float(self.lo):.17g}, "
                                         f"{float(self.hi):.17g}] (sum e^2 = {float(self.mid):.17g})")

    def moved(self, got, e, k=4.0):
        return float(self.mid + k * (self.hi - self.mid))


def sumsq_expect(terms):
    t = np.asarray(terms, dtype=LD).reshape(-1)
    s = np.sum(t * t)
    return Within(np.array([s]), np.array([(t.size + 2) * U * s]))


# ------------------------------------------------------------------------------------------ buffers
class _Out(CC._Out):
    """CC._Out for any storage type: 0xFF bytes are NaN in fp64, fp32 and bf16 alike"""

    def __init__(self, sh, nelem, t, idx=None, init=None):
        self.t, self.nelem = np.dtype(t), nelem
        self.img = np.full(2 * GUARD + nelem * self.t.itemsize, 0xFF, np.uint8)
        if init is not None:
            self.img[GUARD:GUARD + nelem * self.t.itemsize].view(self.t)[idx] = init
        self.sh, self.base = sh, sh.alloc(self.img.size)
        sh.h2d(self.base, self.img)
        self.ptr = self.base + GUARD


class St:
    """the buffers and the outcome of one run of a case"""

    def __init__(self, sh, c, hip, data):
        self.sh, self.c, self.hip, self.d = sh, c, hip, data
        self.keep, self.outs, self.posts, self.tags, self.expect, self.host = [], {}, {}, [], {}, {}

    def inp(self, payload, lead=0):
        b = CC._In(self.sh, np.ascontiguousarray(payload), lead=lead)
        self.keep.append(b)
        return b

    def out(self, name, n, dt="f64", res=None, idx=None, init=None, lead=0):
        """an output of n elements of storage type dt behind `lead` elements that must stay NaN; res: the elements
        the calls must write (default all), idx / init: elements that hold (storage) values beforehand"""
        o = _Out(self.sh, n + lead, NPT[dt], None if idx is None else np.asarray(idx) + lead, init)
        o.ptr += lead * NPT[dt].itemsize
        self.keep.append(o)
        self.outs[name] = (o, (np.arange(n) if res is None else np.asarray(res, dtype=np.int64)) + lead, dt)
        return o

    def finish(self):
        self.sh.sync()
        self.tags += self.sh.route_take()
        for name, (o, _, _) in self.outs.items():
            self.posts[name] = o.download()
        for b in self.keep:
            if isinstance(b, CC._In):
                b.check(self.c["name"])

    def body(self, name):
        """(the self-test) the downloaded result elements, writable, as storage elements"""
        o, res, _ = self.outs[name]
        return self.posts[name][GUARD:-GUARD].view(o.t), res

    def bits(self, name):
        """the result's storage elements, guards and gaps checked"""
        o, res, dt = self.outs[name]
        what = f"{self.c['name']} {name}"
        check_image(what, o.img, self.posts[name], o.t, res)
        return self.posts[name][GUARD:-GUARD].view(o.t)[res]

    def got(self, name):
        dt = self.outs[name][2]
        v = decode(self.bits(name), dt)
        assert not np.any(np.isnan(v)), f"{self.c['name']} {name}: {int(np.sum(np.isnan(v)))} result elements are NaN"
        return v

    def free(self):
        for b in self.keep:
            b.free()
        self.keep = []


def run_case(sh, c, hip, ncu=None, log=None, perturb=None):
    """Runs a case twice on the shim `sh`, compares the two runs bit for bit and checks the second against the
    expectations the op set up (st.expect: output name -> Within / Interval / bytes). perturb(st): the self-test's
    hook on the outcome before it is verified. Returns the route tags."""
    if hip and c.get("dev") and ncu != 256:
        raise CC.Skip(f"{c['name']}: sized for 256 CUs, this device has {ncu}")
    data = DATA[c["op"]](c)
    first = None
    for rep in (0, 1):
        st = St(sh, c, hip, data)
        try:
            sh.route_take()
            OPS[c["op"]](st)
            if rep == 0:
                first = (st.posts, st.host)
                continue
            assert first[0].keys() == st.posts.keys()
            for k in first[0]:
                assert np.array_equal(first[0][k], st.posts[k]), f"{c['name']} {k}: two runs differ in bits"
            for k in first[1]:
                assert np.array_equal(first[1][k].view(np.uint8), st.host[k].view(np.uint8)), \
                    f"{c['name']} {k}: two runs differ in bits"
            if perturb:
                perturb(st)
            verify(st, log)
            if hip:
                check_route(c["name"], c, st.tags)
            return st.tags
        finally:
            st.free()


def verify(st, log=None):
    c = st.c
    for name in st.outs:
        ex = st.expect[name]
        if isinstance(ex, np.ndarray):  # exact, as storage elements
            same = np.array_equal(st.bits(name).view(np.uint8), ex.view(np.uint8))
            _worst(c["family"], 0.0 if same else np.inf)
            assert same, f"{c['name']} {name}: not exact"
        else:
            ex.check(c, name, st.got(name), log)
    for name, arr in st.host.items():
        same = np.array_equal(arr.view(np.uint8), st.expect[name].view(np.uint8))
        _worst(c["family"], 0.0 if same else np.inf)
        assert same, f"{c['name']} {name}: not exact"


# ------------------------------------------------------------------------------------------ K10
def _colblocks(M, K):
    step = max(1, (1 << 20) // M)
    return [(k0, min(K, k0 + step)) for k0 in range(0, K, step)]


def _model(Q, P, k0, k1):
    """(m, a) of the columns k0 .. k1 in long double"""
    if Q.shape[1] <= 4:  # (the long tensors: no long-double matmul)
        m = sum(Q[:, r:r + 1].astype(LD) * P[None, k0:k1, r].astype(LD) for r in range(Q.shape[1]))
        a = sum(np.abs(Q[:, r:r + 1]).astype(LD) * np.abs(P[None, k0:k1, r]).astype(LD) for r in range(Q.shape[1]))
        return m, a
    return Q.astype(LD) @ P[k0:k1].astype(LD).T, np.abs(Q).astype(LD) @ np.abs(P[k0:k1]).astype(LD).T


def spike_at(c):
    M, K = c["M"], c["K"]
    return [(M - 1, K // 2), (M // 2, K - 1), (0, 0), (min(1, M - 1), 128 if K > 128 else K - 1)][c["spike"]]


def rank_data(c):
    """the inputs of a K10 case and the expectation, computed once for both runs (and for the second reference)"""
    rng = np.random.default_rng(c["seed"])
    mode, dt, M, K, R = c["mode"], c["dt"], c["M"], c["K"], c["R"]
    d = dict(Q=None, P=None, Vx=None)
    if mode == 2:
        d["Vx"], d["Vs"] = _stored(vals(rng, c["cls"], (M, K)), dt)
        if c["vcls"] == "spike":
            d["Vx"] = d["Vx"].copy()
            d["Vx"][spike_at(c)] = SPIKE
            d["Vs"] = _stored(d["Vx"], dt)[1]
        d["expect"] = sumsq_expect(d["Vx"])
        return d
    Q, P = vals(rng, c["cls"], (M, R)), vals(rng, c["cls"], (K, R))
    d["Q"], d["P"] = Q, P
    if mode == 0:
        ref, bar = np.empty((M, K), LD), np.empty((M, K), LD)
        for k0, k1 in _colblocks(M, K):
            m, a = _model(Q, P, k0, k1)
            ref[:, k0:k1] = m
            bar[:, k0:k1] = (R + 1) * U * a + UDT[dt] * (np.abs(m) + (R + 1) * U * a)
        d["expect"] = Within(ref, bar)
        return d
    if c["vcls"] == "far":
        Vx = _stored(vals(rng, c["cls"], (M, K)), dt)[0]
    else:
        Vx = np.empty((M, K))
        for k0, k1 in _colblocks(M, K):
            Vx[:, k0:k1] = _stored(_model(Q, P, k0, k1)[0].astype(np.float64), dt)[0]
        if c["vcls"] == "spike":
            Vx[spike_at(c)] = SPIKE
    d["Vx"], d["Vs"] = Vx, _stored(Vx, dt)[1]
    lo = mid = hi = LD(0)
    for k0, k1 in _colblocks(M, K):
        m, a = _model(Q, P, k0, k1)
        e = np.abs(Vx[:, k0:k1].astype(LD) - m)
        delta = (R + 2) * U * a + U * e
        lo, mid, hi = lo + np.sum(np.maximum(e - delta, 0) ** 2), mid + np.sum(e * e), hi + np.sum((e + delta) ** 2)
    n = M * K
    d["expect"] = Interval(lo * (1 - (n + 2) * U), mid, hi * (1 + (n + 2) * U))
    return d


def op_rank(st):
    c, sh, d = st.c, st.sh, st.d
    mode, dt, M, K, R, voff = c["mode"], c["dt"], c["M"], c["K"], c["R"], c.get("voff", 0)
    q = p = None
    if mode != 2:
        q, p = st.inp(d["Q"].reshape(-1, order="F")), st.inp(d["P"].reshape(-1, order="F"))
    if mode == 0:
        v = st.out("V", M * K, dt, lead=voff)
        sh.fill_rank(v.ptr, DT[dt], M, K, q.ptr, p.ptr, R)
        st.expect["V"] = Within(d["expect"].ref.reshape(-1, order="F"), d["expect"].bar.reshape(-1, order="F"))
    else:
        v = st.inp(np.asarray(d["Vs"]).reshape(-1, order="F"), lead=voff)
        o = st.out("out", 1)
        sh.residual_sq(v.ptr, DT[dt], M, K, q.ptr if q else 0, p.ptr if p else 0, R if mode == 1 else 0, o.ptr)
        st.expect["out"] = d["expect"]
    st.finish()


def second_reference(c):
    """The same quantity from numpy in fp64 (BLAS product, numpy's pairwise sums), no device involved, held to the
    same expectation: the bars must not be so tight that a correct fp64 evaluation in another order fails."""
    d = DATA[c["op"]](c)
    if c["op"] == "usumsq":
        x = c["lo"] + (c["hi"] - c["lo"]) * d["u01"]
        got = np.sum(x * x)
    elif c["mode"] == 0:
        got = _stored(d["Q"] @ d["P"].T, c["dt"])[0]
    elif c["mode"] == 1:
        e = d["Vx"] - d["Q"] @ d["P"].T
        got = np.sum(e * e)
    else:
        got = np.sum(d["Vx"] * d["Vx"])
    d["expect"].check(c, "second reference", got)


# ------------------------------------------------------------------------------------------ the generators
def splitmix64(x):
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def global_index(c):
    """gi = row0 + a + g0 r of the shard's elements e = a + l0 r, in uint64"""
    e = np.arange(c["l0"] * c["rest"], dtype=np.uint64)
    with np.errstate(over="ignore"):
        return np.uint64(c["row0"]) + e % np.uint64(c["l0"]) + np.uint64(c["g0"]) * (e // np.uint64(c["l0"]))


def u01(seed, gi):
    h = splitmix64(splitmix64(np.array([seed], dtype=np.uint64)) ^ gi)
    return (h >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def gen_data(c):
    d = dict(u01=u01(c["useed"], global_index(c)))
    lo, dl = LD(c["lo"]), LD(c["hi"]) - LD(c["lo"])
    assert float(dl) == c["hi"] - c["lo"]  # (hi - lo is exact for the ranges of the table)
    x = lo + dl * d["u01"].astype(LD)
    E = 2 * U * (abs(lo) + abs(dl) * d["u01"].astype(LD))
    dt = c.get("dt")
    if c["op"] == "uniform":
        d["expect"] = Within(x, E + UDT[dt] * (np.abs(x) + E))
    elif c["op"] == "noise":
        rng = np.random.default_rng(c["seed"])
        d["V0"], d["V0s"] = _stored(vals(rng, c["cls"], x.shape), dt)
        al = LD(c["alpha"])
        ref = d["V0"].astype(LD) + al * x
        En = abs(al) * E + 2 * U * (np.abs(d["V0"]) + np.abs(al * x))
        d["expect"] = Within(ref, En + UDT[dt] * (np.abs(ref) + En))
    else:
        d["expect"] = sumsq_expect(x)
    return d


def laplacian_ref(gi, ndigits, s):
    """the defining sum over k of D[a_k, b_k] prod_{j != k} [a_j == b_j], D = tridiag(-1, 2, -1) (ops.h)"""
    gi = gi.astype(np.uint64)
    a, b = [], []
    for _ in range(ndigits // 2):
        a.append((gi % np.uint64(s)).astype(np.int64))
        gi = gi // np.uint64(s)
        b.append((gi % np.uint64(s)).astype(np.int64))
        gi = gi // np.uint64(s)
    v = np.zeros(len(gi))
    for k in range(ndigits // 2):
        term = np.where(a[k] == b[k], 2.0, np.where(np.abs(a[k] - b[k]) == 1, -1.0, 0.0))
        for j in range(ndigits // 2):
            if j != k:
                term = term * (a[j] == b[j])
        v += term
    return v


def op_gen(st):
    c, sh, d = st.c, st.sh, st.d
    l0, g0, row0, rest, n = c["l0"], c["g0"], c["row0"], c["rest"], c["l0"] * c["rest"]
    dt = c.get("dt")
    if c["op"] == "uniform":
        v = st.out("V", n, dt)
        sh.fill_uniform(v.ptr, DT[dt], l0, g0, row0, rest, c["useed"], c["lo"], c["hi"])
        st.expect["V"] = d["expect"]
    elif c["op"] == "noise":
        v = st.out("V", n, dt, idx=np.arange(n), init=np.asarray(d["V0s"]).reshape(-1))
        sh.add_uniform_noise(v.ptr, DT[dt], l0, g0, row0, rest, c["useed"], c["lo"], c["hi"], c["alpha"])
        st.expect["V"] = d["expect"]
    elif c["op"] == "usumsq":
        o = st.out("out", 1)
        sh.uniform_sumsq(l0, g0, row0, rest, c["useed"], c["lo"], c["hi"], o.ptr)
        st.expect["out"] = d["expect"]
    else:
        v = st.out("V", n, dt)
        sh.fill_laplacian(v.ptr, DT[dt], l0, g0, row0, rest, c["ndigits"], c["s"])
        st.expect["V"] = encode(laplacian_ref(global_index(c), c["ndigits"], c["s"]), dt)
    st.finish()


# ------------------------------------------------------------------------------------------ layouts and shards
def op_pad(st):
    c, sh = st.c, st.sh
    dt, rows, cols, blk, ld = c["dt"], c["rows"], c["cols"], c["blk"], c["ld"]
    rng = np.random.default_rng(c["seed"])
    src = encode(vals(rng, c["cls"], (rows, cols)), dt)  # src[r, c] at r + rows c
    want = np.zeros((ld, cols // blk, rows), NPT[dt])    # dst[(c % blk) + ld (c / blk + (cols / blk) r)]
    for cc in range(cols):
        want[cc % blk, cc // blk, :] = src[:, cc]
    s = st.inp(src.reshape(-1, order="F"))
    o = st.out("dst", want.size, dt)
    sh.pad_layout(s.ptr, DT[dt], rows, cols, blk, ld, o.ptr)
    st.expect["dst"] = want.reshape(-1, order="F")
    st.finish()


def op_unpack(st):
    c, sh = st.c, st.sh
    dt, s0, rest, blk, P = c["dt"], c["s0"], c["rest"], c["blk"], c["P"]
    t = NPT[dt]
    rng = np.random.default_rng(c["seed"])
    full = encode(vals(rng, c["cls"], (s0, rest)), dt)
    chunk = blk * rest * t.itemsize + c["slack"]  # larger than any shard: NaN filler in between
    stage = np.full(P * chunk, 0xFF, np.uint8)
    for p in range(P):
        shard = full[p * blk:min(s0, (p + 1) * blk)]
        stage[p * chunk:p * chunk + shard.size * t.itemsize] = shard.reshape(-1, order="F").view(np.uint8)
    s = st.inp(stage)
    o = st.out("full", s0 * rest, dt)
    sh.unpack_shards(s.ptr, DT[dt], s0, rest, blk, P, chunk, o.ptr)
    st.expect["full"] = full.reshape(-1, order="F")
    st.finish()


def op_krp(st):
    c, sh = st.c, st.sh
    rows, R, col0, ncols, xld = c["fac"], c["R"], c["col0"], c["ncols"], c.get("xld", 0)
    rng = np.random.default_rng(c["seed"])
    Ws = [vals(rng, c["cls"], (r, R)) for r in rows]
    f = CC._upload_factors(sh, Ws, xld, st.keep)
    J = int(np.prod(rows))
    o = st.out("out", J * ncols)
    sh.krp(o.ptr, f, col0, ncols)
    ref = CC._krp([W[:, col0:col0 + ncols] for W in Ws], LD).reshape(-1, order="F")
    st.expect["out"] = Within(ref, (len(rows) - 1) * U * np.abs(ref))
    st.finish()


def op_shard(st):
    """upload_shard, then download_shard of what it stored"""
    c, sh = st.c, st.sh
    dt, l0, g0, row0, rest = c["dt"], c["l0"], c["g0"], c["row0"], c["rest"]
    rng = np.random.default_rng(c["seed"])
    full = vals(rng, c["cls"], (rest, g0))  # full[c, a]: element a + g0 c of the host tensor
    v = st.out("V", l0 * rest, dt)
    sh.upload_shard(v.ptr, DT[dt], full.reshape(-1), l0, g0, row0, rest)
    stored = encode(full[:, row0:row0 + l0], dt)
    st.expect["V"] = stored.reshape(-1)
    back = np.full((rest, g0), np.nan)
    sh.download_shard(v.ptr, DT[dt], back.reshape(-1), l0, g0, row0, rest)
    want = np.full((rest, g0), np.nan)
    want[:, row0:row0 + l0] = decode(stored, dt)
    st.host["host_full"], st.expect["host_full"] = back, want
    st.finish()


OPS = {"rank": op_rank, "uniform": op_gen, "noise": op_gen, "usumsq": op_gen, "laplacian": op_gen, "pad": op_pad,
       "unpack": op_unpack, "krp": op_krp, "shard": op_shard}
DATA = {k: (lambda c: None) for k in OPS}
DATA.update(rank=rank_data, uniform=gen_data, noise=gen_data, usumsq=gen_data)

# ------------------------------------------------------------------------------------------ the table
CASES = []
_seed = [9000]
_vcls = [0]


def _add(op, family, name, route, why, **kw):
    _seed[0] += 1
    kw.setdefault("cls", "pos" if _seed[0] % 2 else "mix")
    c = dict(op=op, family=family, name=f"{family}:{name}", route=route if isinstance(route, list) else [route],
             why=why, seed=_seed[0], **kw)
    CASES.append(c)
    return c


def rank(mode, dt, M, K, R, why, vcls=None, expect=None, voff=0, tag=""):
    """a K10 case; mode 1 / 2 without a value class take the next of far, at, spike (mode 2: far, spike)"""
    kind, pat, dev = rank_route(mode, dt, M, K, R, aligned=not voff)
    assert expect is None or kind == expect, (mode, dt, M, K, R, kind)
    if mode != 0 and vcls is None:
        _vcls[0] += 1
        vcls = ("far", "at", "spike")[_vcls[0] % 3] if mode == 1 else ("far", "spike")[_vcls[0] % 2]
    name = f"{('fill', 'residual', 'norm')[mode]} {dt} M={M} K={K}" + (f" R={R}" if mode != 2 else "") + \
        (f" {vcls}" if vcls else "") + (" base+1" if voff else "") + tag
    return _add("rank", "rank_" + kind, name, pat, why, mode=mode, dt=dt, M=M, K=K, R=R if mode != 2 else 0, vcls=vcls,
                spike=_seed[0] % 4, voff=voff, dev=dev)


# ---- rank.mfma: fp32 (VEC 4, a tile of 256 rows) and fp64 (VEC 2, 128 rows); K = 131 is 9 column blocks, chunks of 8
# and 1, the last block with 3 live columns
for dt in ("f32", "f64"):
    v, tile = VEC[dt], 64 * VEC[dt]
    for M, why in ((tile + v, "one live lane, dead waves"), (v, "a single vector of rows"), (2 * tile, "two full tiles")):
        rank(0, dt, M, 131, 10, why, expect="mfma")
        for vc in ("far", "at", "spike"):
            rank(1, dt, M, 131, 10, why, vcls=vc, expect="mfma")
        rank(2, dt, M, 131, 0, why, expect="mfma")
    for K in (1, 16, 17):
        rank(0, dt, tile + v, K, 9, "column block edges", expect="mfma")
        rank(1, dt, tile + v, K, 9, "column block edges", expect="mfma")
        rank(2, dt, tile + v, K, 0, "column block edges", expect="mfma")
    for R in (1, 4, 5, 6, 9, 12, 13, 14, 16, 17, 18, 21, 32):  # (R = 10 above) every (MAXRB, REM), and the refusals
        rank(1, dt, tile + v, 131, R, "MAXRB and REM by rank", expect="mfma")
    for R in (1, 12, 13, 16, 17, 32):
        rank(0, dt, tile + v, 131, R, "MAXRB by rank", expect="mfma")
    for mode in (0, 1, 2):
        rank(mode, dt, tile + v, 131, 13, "misaligned base: stream", voff=1, expect="stream")

# ---- rank.split: M = 16 VEC + VEC is two row tiles of 16 VEC rows, the second with one live lane
for dt in ("f32", "f64"):
    M = 17 * VEC[dt]
    for R in (33, 36, 37, 64, 65, 128, 129, 250, 256):  # (33, 36: RB = 9, rbw = 3: wave 3 holds no rank block)
        rank(1, dt, M, 131, R, "MAXRBW, ragged rank blocks", expect="split")
        rank(0, dt, M, 131, R, "MAXRBW, ragged rank blocks", expect="split")
    for mode in (0, 1):
        rank(mode, dt, M, 131, 257, "above 256: any-rank stream", expect="stream")

# ---- rank.stream: M = 259 is two row blocks (the second ragged) and no vector multiple, K = 33 two k-chunks
for dt in ("f32", "f64", "bf16"):
    for R in (1, 16, 17, 32, 33, 64, 65):
        for mode in (0, 1):
            rank(mode, dt, 259, 33, R, "register blocks by rank", expect="stream")
    rank(2, dt, 259, 33, 0, "sum of squares", vcls="far", expect="stream")
    rank(2, dt, 259, 33, 0, "sum of squares", vcls="spike", expect="stream")
for mode in (0, 1, 2):
    rank(mode, "bf16", 512, 131, 10, "bf16 never on MFMA", expect="stream", tag=" aligned")
rank(1, "f32", 3, 32 * 65535 + 1, 2, "kch doubles to 64", vcls="far", expect="stream")


# ---- the generators
def gen(op, name, why, l0, g0, row0, rest, **kw):
    return _add(op, "generators", name, [], why, l0=l0, g0=g0, row0=row0, rest=rest, useed=0x5EED0000 + _seed[0], **kw)


SHARDS = {"inner": (13, 37, 11, 301), "2^40": (7, 2 ** 40, 2 ** 40 - 7, 1000)}
RANGES = ((0.0, 1.0), (0.5, 1.0), (-1.0, 1.0))
for sn, shard in SHARDS.items():
    for i, dt in enumerate(("f32", "f64", "bf16")):
        for j, (lo, hi) in enumerate(RANGES):
            if sn == "inner" or j == i:
                gen("uniform", f"uniform {dt} {sn} [{lo},{hi})", "shard inside the mode", *shard, dt=dt, lo=lo, hi=hi)
        lo, hi = RANGES[(i + 1) % 3]
        gen("noise", f"noise {dt} {sn} [{lo},{hi})", "noise on a shard", *shard, dt=dt, lo=lo, hi=hi, alpha=0.37 * (i + 1))
    for lo, hi in RANGES:
        gen("usumsq", f"sumsq {sn} [{lo},{hi})", "same index set", *shard, lo=lo, hi=hi)
WRAP = (21, 29, 5, 199741)  # 21 * 199741 = 16384 * 256 + 257 elements: the grid-stride loop wraps
gen("uniform", "uniform f32 wrap", "grid-stride wrap", *WRAP, dt="f32", lo=-1.0, hi=1.0)
gen("noise", "noise f32 wrap", "grid-stride wrap", *WRAP, dt="f32", lo=-1.0, hi=1.0, alpha=0.5)
gen("usumsq", "sumsq wrap", "grid-stride wrap", *WRAP, lo=-1.0, hi=1.0)
for s, nd, l0 in ((3, 4, 2), (3, 6, 2), (5, 4, 3), (5, 6, 3)):
    for dt in ("f32", "f64", "bf16"):
        gen("laplacian", f"laplacian {dt} s={s} ndigits={nd}", "odd row0", l0, s, 1, s ** (nd - 1), dt=dt, s=s, ndigits=nd)

# ---- the layouts
for dt in ("f32", "f64", "bf16"):
    for rows in (70, 129):  # blk = 50 in ld = 64, 3 blocks: a 64-column tile of the transposition straddles blocks
        _add("pad", "layouts", f"pad {dt} rows={rows}", [], "tile straddles blocks", dt=dt, rows=rows, cols=150, blk=50,
             ld=64)
    _add("pad", "layouts", f"pad {dt} rows=1", [], "pitched copy", dt=dt, rows=1, cols=150, blk=50, ld=64)
    _add("pad", "layouts", f"pad {dt} blk=ld", [], "no padding", dt=dt, rows=70, cols=128, blk=64, ld=64)
    _add("unpack", "layouts", f"unpack {dt}", [], "short last shard", dt=dt, s0=10, rest=7, blk=4, P=3, slack=64)
for fac, R, col0, ncols, xld in (((37,), 5, 0, 5, 0), ((5, 7), 6, 2, 3, 3), ((3, 4, 5), 4, 1, 3, 2), ((6, 11), 7, 0, 7, 1)):
    _add("krp", "layouts", f"krp nf={len(fac)} J={int(np.prod(fac))} col0={col0} ncols={ncols}/{R}", [],
         "factors, ld, column window", fac=fac, R=R, col0=col0, ncols=ncols, xld=xld)

# ---- the shards
for dt in ("f32", "f64", "bf16"):
    _add("shard", "shards", f"shard {dt}", [], "rows inside the mode", dt=dt, l0=5, g0=13, row0=4, rest=77)
# l0 * rest * 8 bytes = 64 MiB + 16000: the staging loop runs twice, the second time with 1000 columns
_add("shard", "shards", "shard f32 two chunks", [], "staging loop runs twice", dt="f32", l0=2, g0=3, row0=1,
     rest=(64 << 20) // 16 + 1000)

FAMILIES = sorted({c["family"] for c in CASES})
K10 = [c for c in CASES if c["op"] == "rank"]
