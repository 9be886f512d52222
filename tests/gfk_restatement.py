"""CPU restatement of the device's Gulunay f-k densification (kiwi_amd/csrc/kiwi_gfk.hpp): numpy, fp32, in the device's
operation order, so that the GPU tests can ask for bit identity.

What it restates, in the reference's terms:
  * the densified grid and its block cover: gfdb.f90:223-246 (grid), :31-37 (block sizes), :1127-1135 (block ranges);
  * the time window of a block: the union of the spans of its stored traces through allowed_span (:1139-1161, :1313-1330),
    filled like trace_multiply_add_nogrow (sparse_trace.f90:710-800): zeros before a trace, its end value after it;
  * the dispatch of interpolate3d (gfdb.f90:1236-1310), quirks of the unequal-factor path included;
  * gulunay2d / gulunay3d (interpolation.f90:29-311): cosine tapers, the zero-trace insert B, the zero-padded C, the
    decimated D, the noise floor on D's spectrum, the operator fC/fD with its clip, fB*Op/N and the inverse transform;
  * the write-back (gfdb.f90:1188-1226): payload positions that are not stored and lie inside the grid, each with the
    span union of its up-to-four stored corner neighbours.
Decisions the reference leaves open (INTEGRATION.md "Limits"): work arrays it never sets are zeros; a missing stored
trace adds zeros to the field and nothing to a span union, and a position whose neighbours are all missing stays
missing.  The transforms are radix-2 Stockham passes with twiddles from an fp64 table rounded to fp32 (FFTW's own
rounding is out of reach); magnitudes are a scaled hypot and divisions follow Smith's formula.  A spectral bin where fC/fD
is undefined (fD exactly zero, which the noise floor leaves in place when m == 0, or an overflowing quotient) gets no
operator.

Transcendentals on the host side (tapers, the power-of-two length) go through the C library, as the device's host code
does, so both sides see the same bits."""
import ctypes
import ctypes.util
import math

import numpy as np

F32 = np.float32
_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _n, _t in (("cosf", ctypes.c_float), ("logf", ctypes.c_float), ("cos", ctypes.c_double), ("sin", ctypes.c_double)):
    getattr(_libm, _n).restype = _t
    getattr(_libm, _n).argtypes = [_t]

PI_F = F32(3.14159265358979)             # constants.f90:21, a default real
NBLOCKX, NBLOCKX_OVERLAP = 128, 32       # gfdb.f90:31-33
NBLOCKZ, NBLOCKZ_OVERLAP = 32, 8         # gfdb.f90:35-37


def check_factors(nipx, nipz):
    """None if the factors are accepted, else the message the drop-in refuses them with."""
    if nipx < 1 or nipz < 1:
        return "set_database: nipx and nipz must be positive"          # minimizer.f90:143-146
    for name, v, top in (("nipx", nipx, NBLOCKX), ("nipz", nipz, NBLOCKZ)):
        if v > top or v & (v - 1):
            # gulunay2d dies unless the coarse block width divides the fine one (interpolation.f90:55,191)
            return ("set_database: %s must be a power of two up to %d (the interpolation block is %d traces wide)"
                    % (name, top, top))
    return None


def axis_blocking(nip, nblock, overlap):
    """(block, payload, overlap) of one axis, gfdb.f90:225-246."""
    if nip == 1:
        return 1, 1, 0
    return nblock, nblock - overlap, overlap


def next_power_of_two(n):
    """gfdb.f90:1332-1339 in default reals: 2**ceiling(log(real(n))/log(2.))."""
    q = F32(_libm.logf(float(F32(n)))) / F32(_libm.logf(2.0))
    return 2 ** int(math.ceil(float(F32(q))))


def allowed_span(s1, s2, minlength):
    """gfdb.f90:1313-1330."""
    length = s2 - s1 + 1
    if length < minlength:
        length = minlength
    lengthp = next_power_of_two(length)
    s1 = s1 - (lengthp - length) // 2
    return s1, s1 + lengthp - 1


def window(s1, s2):
    """allowed_span(span, min(64, int(1.2*(span(2)-span(1))))) and ntmargin = int(0.1*(span(2)-span(1))) of the new
    span (gfdb.f90:1159-1173), default-real arithmetic."""
    minlen = min(64, int(F32(s2 - s1) * F32(1.2)))
    w1, w2 = allowed_span(s1, s2, minlen)
    return w1, w2 - w1 + 1, int(F32(w2 - w1) * F32(0.1))


class Plan:
    """Block cover of a densification: per block its window and the dense positions it writes (all 1-based in the dense
    grid, like the reference)."""

    def __init__(self, nx, nz, ng, first, nsamp, nipx, nipz):
        self.nx, self.nz, self.ng, self.nipx, self.nipz = nx * nipx, nz * nipz, ng, nipx, nipz
        self.bx, self.px, self.ox = axis_blocking(nipx, NBLOCKX, NBLOCKX_OVERLAP)
        self.bz, self.pz, self.oz = axis_blocking(nipz, NBLOCKZ, NBLOCKZ_OVERLAP)
        present = nsamp > 0
        self.blocks = []
        for ibx in range((self.nx + self.px - 1) // self.px):
            for ibz in range((self.nz + self.pz - 1) // self.pz):
                self.blocks.append(self._block(ibx, ibz, first, nsamp, present))

    def get_index(self, i, n, nip):
        """Stored neighbour of dense 1-based position i (edges repeated, gfdb.f90:1141-1142), as a coarse 0-based index."""
        return (min(max(i, 1), n) - 1) // nip

    def _block(self, ibx, ibz, first, nsamp, present):
        ixfirst = ibx * self.px + 1 - self.ox // 2
        izfirst = ibz * self.pz + 1 - self.oz // 2
        b = dict(ixfirst=ixfirst, izfirst=izfirst, T=0, writes=[])
        # stored (local) positions: their coarse source and the span the write-back sees -- the loop over components
        # overwrites spans(:,iz,ix), so it holds the last component's (gfdb.f90:1147-1156)
        src, spans = {}, {}
        lo, hi = None, None
        for lx in range(0, self.bx, self.nipx):
            for lz in range(0, self.bz, self.nipz):
                cx = self.get_index(ixfirst + lx, self.nx, self.nipx)
                cz = self.get_index(izfirst + lz, self.nz, self.nipz)
                src[lx, lz] = (cx, cz)
                for ig in range(self.ng):
                    if present[cx, cz, ig]:
                        f, n = int(first[cx, cz, ig]), int(nsamp[cx, cz, ig])
                        lo = f if lo is None else min(lo, f)
                        hi = f + n - 1 if hi is None else max(hi, f + n - 1)
                if present[cx, cz, self.ng - 1]:
                    f, n = int(first[cx, cz, self.ng - 1]), int(nsamp[cx, cz, self.ng - 1])
                    spans[lx, lz] = (f, f + n - 1)
        b["src"] = src
        if lo is None:                 # no stored trace at all: nothing is written (decision b)
            return b
        w0, T, ntm = window(lo, hi)
        if T <= 1:                     # gfdb.f90:1163
            return b
        b.update(w0=w0, T=T, ntmargin=ntm)
        for lz in range(self.oz // 2, self.bz - self.oz // 2):
            for lx in range(self.ox // 2, self.bx - self.ox // 2):
                ix, iz = ixfirst + lx, izfirst + lz
                if (ix - 1) % self.nipx == 0 and (iz - 1) % self.nipz == 0:
                    continue
                if ix < 1 or ix > self.nx or iz < 1 or iz > self.nz:
                    continue
                ax = (lx // self.nipx) * self.nipx
                az = (lz // self.nipz) * self.nipz
                corners = [(ax, az)]
                if ax + self.nipx < self.bx:
                    corners.append((ax + self.nipx, az))
                if az + self.nipz < self.bz:
                    corners.append((ax, az + self.nipz))
                if ax + self.nipx < self.bx and az + self.nipz < self.bz:
                    corners.append((ax + self.nipx, az + self.nipz))
                got = [spans[k] for k in corners if k in spans]
                if not got:
                    continue
                d0 = min(s[0] for s in got)
                d1 = max(s[1] for s in got)
                b["writes"].append((ix, iz, lx, lz, d0, d1))
        return b


# ---------------------------------------------------------------------------------------------------- transforms
_tw = {}


def twiddles(n):
    """exp(-2 pi i k / n), k < n/2: fp64 through the C library, rounded to fp32."""
    if n not in _tw:
        k = np.arange(max(n // 2, 1))
        re = np.array([_libm.cos(2.0 * math.pi * float(j) / float(n)) for j in k], np.float64)
        im = np.array([-_libm.sin(2.0 * math.pi * float(j) / float(n)) for j in k], np.float64)
        _tw[n] = (re.astype(F32), im.astype(F32))
    return _tw[n]


def fft_last(re, im, inverse=False):
    """Unnormalised radix-2 Stockham transform along the last axis (sign -1 forward, +1 inverse); every product and sum
    rounded on its own.  Pass with stride s over n = N/s: a = x[q+s*p], b = x[q+s*(p+n/2)],
    y[q+s*2p] = a+b, y[q+s*(2p+1)] = (a-b)*w^(p*s)."""
    lead = re.shape[:-1]
    N = re.shape[-1]
    twr, twi = twiddles(N)
    if inverse:
        twi = -twi
    n, s = N, 1
    while n > 1:
        m = n // 2
        xr = re.reshape(lead + (2, m, s))
        xi = im.reshape(lead + (2, m, s))
        ar, br, ai, bi = xr[..., 0, :, :], xr[..., 1, :, :], xi[..., 0, :, :], xi[..., 1, :, :]
        wr = twr[np.arange(m) * s][:, None]
        wi = twi[np.arange(m) * s][:, None]
        sr, si = ar + br, ai + bi
        dr, di = ar - br, ai - bi
        tr = dr * wr - di * wi
        ti = dr * wi + di * wr
        re = np.stack([sr, tr], axis=-2).reshape(lead + (N,))
        im = np.stack([si, ti], axis=-2).reshape(lead + (N,))
        n, s = m, s * 2
    return re, im


def fft_axis(re, im, axis, inverse=False):
    if re.shape[axis] == 1:
        return re, im
    r, i = fft_last(np.ascontiguousarray(np.moveaxis(re, axis, -1)), np.ascontiguousarray(np.moveaxis(im, axis, -1)),
                    inverse)
    return np.moveaxis(r, -1, axis), np.moveaxis(i, -1, axis)


def habs(re, im):
    """|z| as a scaled hypot: M * sqrt(1 + (m/M)^2), M = max(|re|,|im|), m = min; 0 for z = 0."""
    a, b = np.abs(re), np.abs(im)
    mx, mn = np.maximum(a, b), np.minimum(a, b)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = mn / mx
        v = mx * np.sqrt(F32(1) + r * r)
    return np.where(mx == 0, F32(0), v).astype(F32)


def cdiv(ar, ai, br, bi):
    """(a)/(b) by Smith's formula."""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        big = np.abs(br) >= np.abs(bi)
        r1 = bi / br
        d1 = br + bi * r1
        re1 = (ar + ai * r1) / d1
        im1 = (ai - ar * r1) / d1
        r2 = br / bi
        d2 = br * r2 + bi
        re2 = (ar * r2 + ai) / d2
        im2 = (ai * r2 - ar) / d2
    return np.where(big, re1, re2).astype(F32), np.where(big, im1, im2).astype(F32)


def taper_weight(i, margin, l):
    """1 - cos(2 pi (i / (2*margin/l))) as interpolation.f90:67-81 writes it, default reals."""
    den = F32(F32(2.0) * F32(margin)) / F32(l)
    q = F32(i) / den
    return F32(F32(1.0) - F32(_libm.cosf(float(F32(F32(2.0) * PI_F) * q))))


def taper_tables(S, margin, l):
    """(count, start weights, end weights) of one axis of length S."""
    cnt = margin // l
    ws = np.ones(S, F32)
    we = np.ones(S, F32)
    for x in range(1, cnt + 1):
        if 1 <= x <= S:
            ws[x - 1] = taper_weight(x - 1, margin, l)
    for x in range(S - cnt + 1, S + 1):
        if 1 <= x <= S:
            we[x - 1] = taper_weight(S - x, margin, l)
    return cnt, ws, we


def _apply_taper(A, axis, S, margin, l):
    cnt, ws, we = taper_tables(S, margin, l)
    if cnt <= 0:
        return A
    shape = [1] * A.ndim
    shape[axis] = S
    idx = np.arange(S).reshape(shape)
    A = np.where(idx < cnt, (A * ws.reshape(shape)) / F32(2), A).astype(F32)
    A = np.where(idx >= S - cnt, (A * we.reshape(shape)) / F32(2), A).astype(F32)
    return A


def gulunay_pass(A, lx, lz, mx, mz, mt):
    """One gulunay2d (lx or lz == 1) or gulunay3d (lx == lz) call on a batch of fields A[f, x, z, t] -> [f, l*x, l*z, t]."""
    A = np.array(A, F32)
    Fn, Sx, Sz, T = A.shape
    l = max(lx, lz)
    Kx, Kz = Sx * lx, Sz * lz
    H = T // 2 + 1
    # tapers in the reference's order: distance, depth, time (each a multiply, then / 2)
    if lx > 1:
        A = _apply_taper(A, 1, Sx, mx, l)
    if lz > 1:
        A = _apply_taper(A, 2, Sz, mz, l)
    A = _apply_taper(A, 3, T, mt, l)
    # time transforms of the input columns: length T (for B) and l*T zero-padded (for C and D), rows 0..T/2 kept
    zero = np.zeros_like(A)
    bre, bim = fft_last(A, zero)
    Ap = np.concatenate([A, np.zeros((Fn, Sx, Sz, (l - 1) * T), F32)], axis=3)
    cre, cim = fft_last(Ap, np.zeros_like(Ap))
    bre, bim, cre, cim = bre[..., :H], bim[..., :H], cre[..., :H], cim[..., :H]
    fB = [np.zeros((Fn, Kx, Kz, H), F32) for _ in range(2)]
    fC = [np.zeros((Fn, Kx, Kz, H), F32) for _ in range(2)]
    fD = [np.zeros((Fn, Kx, Kz, H), F32) for _ in range(2)]
    fB[0][:, ::lx, ::lz], fB[1][:, ::lx, ::lz] = bre, bim
    fC[0][:, :Sx, :Sz], fC[1][:, :Sx, :Sz] = cre, cim
    fD[0][:, :Sx:lx, :Sz:lz] = cre[:, ::lx, ::lz]
    fD[1][:, :Sx:lx, :Sz:lz] = cim[:, ::lx, ::lz]
    for arr in (fB, fC, fD):
        arr[0], arr[1] = fft_axis(arr[0], arr[1], 2)
        arr[0], arr[1] = fft_axis(arr[0], arr[1], 1)
    # noise floor, operator, clip, product (interpolation.f90:117-146, :270-300)
    dre, dim_ = fD
    m = F32(0.01) * habs(dre[..., H - 1], dim_[..., H - 1]).reshape(Fn, -1).max(axis=1)
    m = m.astype(F32)[:, None, None, None]
    a = habs(dre, dim_)
    dre = np.where(a < m / F32(1000), m, dre).astype(F32)
    a = habs(dre, dim_)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = (m / a).astype(F32)
    low = a < m
    with np.errstate(invalid="ignore"):
        dre = np.where(low, r * dre, dre).astype(F32)
        dim_ = np.where(low, r * dim_, dim_).astype(F32)
    # a zero denominator (m == 0 leaves it in place) or an overflowing quotient: no operator in that bin
    ore, oim = cdiv(fC[0], fC[1], dre, dim_)
    undefined = ((dre == 0) & (dim_ == 0)) | ~np.isfinite(ore) | ~np.isfinite(oim)
    ore = np.where(undefined, F32(0), ore).astype(F32)
    oim = np.where(undefined, F32(0), oim).astype(F32)
    clip = F32(lx * lz)
    a = habs(ore, oim)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = (clip / a).astype(F32)
    hi = a > clip
    with np.errstate(invalid="ignore"):
        ore = np.where(hi, r * ore, ore).astype(F32)
        oim = np.where(hi, r * oim, oim).astype(F32)
    a = habs(ore, oim)
    lo = a < clip * F32(0.5)
    ore = np.where(lo, F32(0), ore).astype(F32)
    oim = np.where(lo, F32(0), oim).astype(F32)
    N = F32(T * Kx * Kz)
    ire = (fB[0] * ore - fB[1] * oim) / N
    iim = (fB[0] * oim + fB[1] * ore) / N
    # back: distance, depth, then the half spectrum in time (Hermitian extension, complex transform, real part)
    ire, iim = fft_axis(ire, iim, 1, inverse=True)
    ire, iim = fft_axis(ire, iim, 2, inverse=True)
    fre = np.zeros((Fn, Kx, Kz, T), F32)
    fim = np.zeros((Fn, Kx, Kz, T), F32)
    fre[..., :H], fim[..., :H] = ire, iim
    if T > 2:
        fre[..., H:] = ire[..., 1:H - 1][..., ::-1]
        fim[..., H:] = -iim[..., 1:H - 1][..., ::-1]
    out, _ = fft_last(fre, fim, inverse=True)
    return out.astype(F32)


def interpolate3d(fin, nipx, nipz, mt, mx, mz):
    """gfdb.f90:1236-1310 on a batch of fields fin[f, x, z, t]."""
    if nipz == 1:
        return gulunay_pass(fin, nipx, 1, mx, 0, mt)
    if nipx == 1:
        return gulunay_pass(fin, 1, nipz, 0, mz, mt)
    if nipx == 4 and nipz == 4:
        mid = gulunay_pass(fin, 2, 2, mx // 2, mz // 2, mt)
        return gulunay_pass(mid, 2, 2, mx, mz, mt)
    if nipx == nipz:
        return gulunay_pass(fin, nipx, nipz, mx, mz, mt)
    Fn, Sx, Sz, T = fin.shape
    Kx, Kz = Sx * nipx, Sz * nipz
    # horizontal pass per stored depth row
    hin = np.ascontiguousarray(np.transpose(fin, (0, 2, 1, 3))).reshape(Fn * Sz, Sx, 1, T)
    hout = gulunay_pass(hin, nipx, 1, mx, 0, mt).reshape(Fn, Sz, Kx, T)
    # vertical pass per output column; the input column is chosen with mod(ix_in-1, nipx) (gfdb.f90:1301) and the
    # distance margin tapers depth (:1306)
    vin = np.empty((Fn, Kx, Sz, T), F32)
    for xo in range(Kx):
        xi = xo // nipx
        vin[:, xo] = fin[:, xi] if xi % nipx == 0 else hout[:, :, xo]
    vout = gulunay_pass(vin.reshape(Fn * Kx, 1, Sz, T), 1, nipz, 0, mx, mt)
    return vout.reshape(Fn, Kx, Kz, T)


def gather(plan, b, data, first, nsamp):
    """field_orig of a block for every component: [ng, x, z, t] (gfdb.f90:1169-1186)."""
    T, w0 = b["T"], b["w0"]
    Sx, Sz = plan.bx // plan.nipx, plan.bz // plan.nipz
    out = np.zeros((plan.ng, Sx, Sz, T), F32)
    t = w0 + np.arange(T)
    for (lx, lz), (cx, cz) in b["src"].items():
        for ig in range(plan.ng):
            n = int(nsamp[cx, cz, ig])
            if n <= 0:
                continue
            k = t - int(first[cx, cz, ig])
            row = np.asarray(data[cx, cz, ig, :n], F32)
            v = np.where(k < 0, F32(0), row[np.clip(k, 0, n - 1)]).astype(F32)
            out[ig, lx // plan.nipx, lz // plan.nipz] = F32(0) + v
    return out


def densify(gf, nipx, nipz):
    """The densified database: dict like make_gfdb's (data[nx', nz', ng, L'], first, nsamp, dx, dz, ...)."""
    msg = check_factors(nipx, nipz)
    if msg:
        raise ValueError(msg)
    data, first, nsamp = gf["data"], gf["first"], gf["nsamp"]
    nx, nz, ng, L = data.shape
    plan = Plan(nx, nz, ng, first, nsamp, nipx, nipz)
    traces = {}
    for b in plan.blocks:
        if not b["writes"]:
            continue
        fin = gather(plan, b, data, first, nsamp)
        out = interpolate3d(fin, nipx, nipz, b["ntmargin"], plan.ox // 2, plan.oz // 2)
        for (ix, iz, lx, lz, d0, d1) in b["writes"]:
            for ig in range(ng):
                traces[ix - 1, iz - 1, ig] = (d0, out[ig, lx, lz, d0 - b["w0"]:d1 - b["w0"] + 1])
    NX, NZ = nx * nipx, nz * nipz
    dfirst = np.zeros((NX, NZ, ng), np.int32)
    dn = np.zeros((NX, NZ, ng), np.int32)
    lmax = max(1, int(nsamp.max()), max((len(v[1]) for v in traces.values()), default=1))
    dd = np.zeros((NX, NZ, ng, lmax), F32)
    dfirst[::nipx, ::nipz] = first
    dn[::nipx, ::nipz] = nsamp
    dd[::nipx, ::nipz, :, :min(L, lmax)] = data[..., :min(L, lmax)]
    for (ix, iz, ig), (f, v) in traces.items():
        dfirst[ix, iz, ig] = f
        dn[ix, iz, ig] = len(v)
        dd[ix, iz, ig, :len(v)] = v
    return dict(dt=gf["dt"], dx=F32(F32(gf["dx"]) / F32(nipx)), dz=F32(F32(gf["dz"]) / F32(nipz)),
                firstx=gf["firstx"], firstz=gf["firstz"], data=dd, first=dfirst, nsamp=dn)
