"""float64 numpy restatement of cy_find_peaks (include/caesar_yolo_hip.h, "residual peaks").

    u(p)      sign * map[p] (fp32, exact), pixel index i = iy * MW + ix
    valid(p)  u(p) non-zero and finite;  noisy(p)  rms[p] finite and > 0
    above(p)  valid, noisy and (double)u(p) >= k_sigma * (double)rms[p]
    rank      p outranks q when u(p) > u(q), or u(p) == u(q) and i(p) < i(q)
    N(p)      |qx - px| <= radius and |qy - py| <= radius inside the image, p included
    peak      above(p) and p outranks every valid q != p of N(p)
    row       x y v rms snr npix nabove sum sw swx swy reserved (lib.PEAK_NAMES), rows in increasing (y, x)

find_peaks() works on whole shifted arrays; brute_force() is the same definition as four nested loops, kept apart so that each
checks the other (tests/test_peaks_cpu.py)."""
import numpy as np

FIELDS = 12
SUMS = (7, 8, 9, 10)                   # sum sw swx swy: the fields whose value depends on the order of a float64 sum


def _planes(m, rms, k_sigma, sign):
    m = np.asarray(m, np.float32)
    rms = np.asarray(rms, np.float32)
    assert m.ndim == 2 and m.shape == rms.shape and sign in (1, -1)
    u = m if sign == 1 else -m
    with np.errstate(all="ignore"):
        valid = (u != 0) & np.isfinite(u)
        noisy = np.isfinite(rms) & (rms > 0)
        above = valid & noisy & (u.astype(np.float64) >= float(k_sigma) * rms.astype(np.float64))
    return m, rms, u, valid, above


def _shifted(a, dy, dx, fill):
    """a[y + dy, x + dx] where that lies inside the image, else fill."""
    H, W = a.shape
    out = np.full(a.shape, fill, a.dtype)
    ys, yd = slice(max(dy, 0), H + min(dy, 0)), slice(max(-dy, 0), H + min(-dy, 0))
    xs, xd = slice(max(dx, 0), W + min(dx, 0)), slice(max(-dx, 0), W + min(-dx, 0))
    out[yd, xd] = a[ys, xs]
    return out


def find_peaks(m, rms, k_sigma=5.0, radius=2, sign=1):
    """-> (rows float64 [n, FIELDS], abs_terms float64 [n, 4]: the sums of |term| of sum, sw, swx, swy, for the bound of a
    reordered float64 sum)."""
    m, rms, u, valid, above = _planes(m, rms, k_sigma, sign)
    R = int(radius)
    shifts = [(dy, dx) for dy in range(-R, R + 1) for dx in range(-R, R + 1)]
    beaten = np.zeros(m.shape, bool)
    with np.errstate(all="ignore"):
        for dy, dx in shifts:
            if dy == 0 and dx == 0:
                continue
            uq, vq = _shifted(u, dy, dx, np.float32(0)), _shifted(valid, dy, dx, False)
            first = dy < 0 or (dy == 0 and dx < 0)                # q comes before p in row-major order
            beaten |= vq & ((uq > u) | ((uq == u) & first))
    peak = above & ~beaten
    ys, xs = np.nonzero(peak)                                     # row-major: increasing (y, x)
    n = ys.size
    rows, absum = np.zeros((n, FIELDS), np.float64), np.zeros((n, 4), np.float64)
    if n == 0:
        return rows, absum
    ud = np.where(valid, u, np.float32(0)).astype(np.float64)
    for dy, dx in shifts:
        uq = _shifted(ud, dy, dx, 0.0)[ys, xs]
        vq = _shifted(valid, dy, dx, False)[ys, xs]
        aq = _shifted(above, dy, dx, False)[ys, xs]
        w = np.maximum(uq, 0.0)
        rows[:, 5] += vq
        rows[:, 6] += aq
        rows[:, 7] += uq
        rows[:, 8] += w
        rows[:, 9] += w * dx
        rows[:, 10] += w * dy
        absum += np.stack([np.abs(uq), w, w * abs(dx), w * abs(dy)], 1)
    rows[:, 0], rows[:, 1] = xs, ys
    rows[:, 2], rows[:, 3] = m[ys, xs].astype(np.float64), rms[ys, xs].astype(np.float64)
    rows[:, 4] = u[ys, xs].astype(np.float64) / rows[:, 3]
    return rows, absum


def brute_force(m, rms, k_sigma=5.0, radius=2, sign=1):
    """The definition pixel by pixel, in Python floats.  -> rows float64 [n, FIELDS]."""
    m, rms, u, valid, above = _planes(m, rms, k_sigma, sign)
    H, W = m.shape
    R = int(radius)
    out = []
    for py in range(H):
        for px in range(W):
            if not above[py, px]:
                continue
            up, is_peak = float(u[py, px]), True
            npix = nabove = 0
            tot = sw = swx = swy = 0.0
            for qy in range(max(py - R, 0), min(py + R, H - 1) + 1):
                for qx in range(max(px - R, 0), min(px + R, W - 1) + 1):
                    if not valid[qy, qx]:
                        continue
                    uq = float(u[qy, qx])
                    if (qy, qx) != (py, px) and (uq > up or (uq == up and qy * W + qx < py * W + px)):
                        is_peak = False
                    npix += 1
                    nabove += int(above[qy, qx])
                    w = max(uq, 0.0)
                    tot, sw, swx, swy = tot + uq, sw + w, swx + w * (qx - px), swy + w * (qy - py)
            if is_peak:
                out.append([px, py, float(m[py, px]), float(rms[py, px]), up / float(rms[py, px]), npix, nabove, tot, sw, swx, swy, 0.0])
    return np.array(out, np.float64).reshape(-1, FIELDS)


def sum_bound(rows, absum):
    """[n, 4]: 2 m 2^-53 sum|t_i| for the four order-dependent sums of every row, m = npix terms (the bound tests/test_gpu_islands.py
    derives for two float64 sums of the same m terms in different orders: each is within (m - 1) u sum|t_i| of the exact sum)."""
    return 2.0 * rows[:, 5:6] * 2.0 ** -53 * absum
