"""Restatement of spec S21, the coarse-to-fine census optical flow, in numpy.

Integer only, so the GPU (cart_optical_flow_pyramid) has to match it bit for bit, level by level.  Written from the spec, per
candidate over whole images with gathers -- not per tile like the kernel.  Census features (S2) come from np_ref.
"""
import numpy as np

import np_ref as N

MIN_W, MIN_H = 24, 16   # a level is built only while it is at least this large


def level_sizes(w, h, levels):
    """-> [(w_l, h_l)] of the levels S21 builds for a w x h frame, level 0 first."""
    sizes = [(w, h)]
    while len(sizes) < levels:
        nw, nh = (sizes[-1][0] + 1) >> 1, (sizes[-1][1] + 1) >> 1
        if nw < MIN_W or nh < MIN_H:
            break
        sizes.append((nw, nh))
    return sizes


def downsample(img):
    """(a + b + c + d + 2) >> 2 over 2x2 blocks, reads clamped to the last column / row."""
    h, w = img.shape
    ys = np.minimum(2 * np.arange((h + 1) >> 1)[:, None] + np.array([0, 1])[None, :], h - 1)   # [h2][2]
    xs = np.minimum(2 * np.arange((w + 1) >> 1)[:, None] + np.array([0, 1])[None, :], w - 1)
    g = img.astype(np.uint32)
    s = sum(g[ys[:, dy]][:, xs[:, dx]] for dy in (0, 1) for dx in (0, 1))
    return ((s + 2) >> 2).astype(np.uint8)


def pyramid(gray, levels):
    out = [np.ascontiguousarray(gray, np.uint8)]
    for _ in level_sizes(gray.shape[1], gray.shape[0], levels)[1:]:
        out.append(downsample(out[-1]))
    return out


def _popcount(x):
    x = x.astype(np.uint32)
    x = x - ((x >> np.uint32(1)) & np.uint32(0x55555555))
    x = (x & np.uint32(0x33333333)) + ((x >> np.uint32(2)) & np.uint32(0x33333333))
    x = (x + (x >> np.uint32(4))) & np.uint32(0x0F0F0F0F)
    return ((x * np.uint32(0x01010101)) >> np.uint32(24)).astype(np.int64)


def window_cost(cen_c, cen_p, du, dv, block):
    """Cost of every pixel p for ITS displacement (du[p], dv[p]): the sum over the window positions q inside the image of
    popcount(cenC(q) ^ cenP(q - d(p))), cenP = 0 outside the image."""
    h, w = cen_c.shape
    yy, xx = np.mgrid[0:h, 0:w]
    cost = np.zeros((h, w), np.int64)
    for dy in range(-block, block + 1):
        for dx in range(-block, block + 1):
            qy, qx = yy + dy, xx + dx
            q_in = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
            sy, sx = qy - dv, qx - du
            s_in = (sy >= 0) & (sy < h) & (sx >= 0) & (sx < w)
            cc = cen_c[np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)]
            pp = np.where(s_in, cen_p[np.clip(sy, 0, h - 1), np.clip(sx, 0, w - 1)], np.uint32(0))
            cost += np.where(q_in, _popcount(cc ^ pp), 0)
    return cost


def search(cen_c, cen_p, pu, pv, radius, block):
    """Winner among (pu + u, pv + v), |u|, |v| <= radius: starts as the prior, replaced only by a strictly smaller cost,
    v outer and u inner, both ascending.  -> int64 [h][w][2] in pixels."""
    best = window_cost(cen_c, cen_p, pu, pv, block)
    bu, bv = pu.copy(), pv.copy()
    for v in range(-radius, radius + 1):
        for u in range(-radius, radius + 1):
            c = window_cost(cen_c, cen_p, pu + u, pv + v, block)
            upd = c < best
            best = np.where(upd, c, best)
            bu = np.where(upd, pu + u, bu)
            bv = np.where(upd, pv + v, bv)
    return np.stack([bu, bv], axis=-1)


def median_flow(f):
    return np.stack([N.median3x3(f[..., 0]), N.median3x3(f[..., 1])], axis=-1)


def pyramid_flow(gray_cur, gray_prev, levels=4, radius=4, refine_radius=2, block=2, median=1, want_levels=False):
    """S21 -> int16 [h][w][2] S10.5 flow; with want_levels also (level images cur, level images prev, level flows in pixels
    -- after the median when it is on)."""
    pc, pp = pyramid(gray_cur, levels), pyramid(gray_prev, levels)
    n = len(pc)
    flows = [None] * n
    for l in range(n - 1, -1, -1):
        cc, cp = N.census(pc[l]), N.census(pp[l])
        h, w = cc.shape
        if l == n - 1:
            zero = np.zeros((h, w), np.int64)
            f = search(cc, cp, zero, zero, radius, block)
        else:
            yy, xx = np.mgrid[0:h, 0:w]
            prior = 2 * flows[l + 1][yy >> 1, xx >> 1]
            f = search(cc, cp, prior[..., 0], prior[..., 1], refine_radius, block)
        flows[l] = median_flow(f) if median else f
    out = (flows[0] * 32).astype(np.int16)
    if want_levels:
        return out, pc, pp, [f.astype(np.int16) for f in flows]
    return out
