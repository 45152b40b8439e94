"""TEST INFRASTRUCTURE ONLY -- the CLAHE ingest stage's rule (include/klt_gpu.h, "CLAHE ingest stage") in plain
numpy, as the header states it: integer arithmetic only, so the device equals it byte for byte.  And the frames and seeded trials the
tests run it on."""
import numpy as np


def clip_q8_of(clip_limit):
    """the clip limit times 256, rounded; None or 0: no clipping (params.equalize_params_from_tc)"""
    return 0 if not clip_limit else int(round(float(clip_limit) * 256.0))


def edges(n, tiles):
    """x_k = (k * n) // tiles, k = 0 .. tiles"""
    return (np.arange(tiles + 1, dtype=np.int64) * n) // tiles


def equalisable(ncols, nrows, tiles_x, tiles_y):
    """the tile grid fits the frame and the per-pixel division is a 32-bit one: the largest Dx * Dy * 255 below 2^32"""
    if tiles_x > ncols or tiles_y > nrows:
        return False
    widest = []
    for n, t in ((ncols, tiles_x), (nrows, tiles_y)):
        c = edges(n, t)[:-1] + edges(n, t)[1:]
        widest.append(int(np.diff(c).max()) if t > 1 else 1)
    return widest[0] * widest[1] * 255 < 2 ** 32


def redistributed_histogram(tile, clip_q8):
    """step 2 up to the bins: the tile's 256-bin histogram, clipped and redistributed (int64)"""
    h = np.bincount(tile.ravel(), minlength=256).astype(np.int64)
    if clip_q8 > 0:
        area = tile.size
        cap = max(1, (clip_q8 * area) >> 16)
        excess = int(np.maximum(h - cap, 0).sum())
        h = np.minimum(h, cap) + excess // 256
        r = excess % 256
        if r:
            h[(np.arange(r, dtype=np.int64) * 256) // r] += 1
    return h


def tile_lut(tile, clip_q8):
    """step 2: lut[b] = (cdf[b] * 255 + A // 2) // A"""
    area = tile.size
    cdf = np.cumsum(redistributed_histogram(tile, clip_q8))
    return ((cdf * 255 + area // 2) // area).astype(np.int64)


def luts(img, tiles_x, tiles_y, clip_q8):
    """[tiles_y][tiles_x][256]"""
    nrows, ncols = img.shape
    xe, ye = edges(ncols, tiles_x), edges(nrows, tiles_y)
    out = np.zeros((tiles_y, tiles_x, 256), np.int64)
    for j in range(tiles_y):
        for i in range(tiles_x):
            out[j, i] = tile_lut(img[ye[j]:ye[j + 1], xe[i]:xe[i + 1]], clip_q8)
    return out


def axis_weights(n, tiles):
    """step 3 for every pixel of an axis: (first tile, second tile, w, D)"""
    e = edges(n, tiles)
    c = e[:-1] + e[1:]                                       # C_k, k = 0 .. tiles - 1
    p = 2 * np.arange(n, dtype=np.int64) + 1
    count = np.searchsorted(c, p, side="right")              # centres at or left of the pixel
    inner = (count >= 1) & (count < tiles)
    k = np.clip(count - 1, 0, tiles - 1)
    first = np.where(count == 0, 0, k)
    second = np.where(inner, k + 1, first)
    k2 = np.minimum(k + 1, tiles - 1)
    w = np.where(inner, p - c[k], 0)
    d = np.where(inner, c[k2] - c[k], 1)
    return first, second, w, d


def clahe(img, tiles_x=8, tiles_y=8, clip_q8=768):
    """the rule on a 2-D uint8 array -> uint8 array of the same shape"""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 2
    nrows, ncols = img.shape
    assert equalisable(ncols, nrows, tiles_x, tiles_y)
    lut = luts(img, tiles_x, tiles_y, clip_q8)
    x0, x1, wx, dx = axis_weights(ncols, tiles_x)
    y0, y1, wy, dy = axis_weights(nrows, tiles_y)
    v = img.astype(np.int64)
    Y0, Y1, WY, DY = y0[:, None], y1[:, None], wy[:, None], dy[:, None]
    X0, X1, WX, DX = x0[None, :], x1[None, :], wx[None, :], dx[None, :]
    d = DX * DY
    num = (lut[Y0, X0, v] * (DX - WX) * (DY - WY) + lut[Y0, X1, v] * WX * (DY - WY)
           + lut[Y1, X0, v] * (DX - WX) * WY + lut[Y1, X1, v] * WX * WY + d // 2)
    out = num // d
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def darken_left_half(img):
    """the issue's low-contrast frame: the left half squeezed to v * 0.08 + 5, truncated"""
    out = np.array(img, np.uint8)
    half = out.shape[1] // 2
    out[:, :half] = (out[:, :half] * 0.08 + 5).astype(np.uint8)
    return out


# ------------------------------------------------------------------------------------------------------------------------ frames
def constant_frame(ncols, nrows, value=77):
    return np.full((nrows, ncols), value, np.uint8)


def two_bin_frame(ncols, nrows, seed=5):
    """all mass in two bins, so that the clipped excess is large and its remainder is spread"""
    rs = np.random.RandomState(seed)
    return np.where(rs.rand(nrows, ncols) < 0.37, 19, 203).astype(np.uint8)


def random_frame(ncols, nrows, seed):
    """a smooth ramp plus noise plus flat patches: runs of equal neighbours and busy stretches in one frame"""
    rs = np.random.RandomState(seed)
    ys, xs = np.mgrid[0:nrows, 0:ncols]
    f = (xs * 3 + ys * 2) % 256 + rs.randint(-20, 21, (nrows, ncols))
    f[: max(1, nrows // 3), : max(1, ncols // 2)] = rs.randint(0, 256)
    return np.clip(f, 0, 255).astype(np.uint8)


def trial(seed):
    """one seeded draw: (frame, tiles_x, tiles_y, clip_q8, pitch) with a frame up to 200 x 150 that is equalisable under the tiles"""
    rs = np.random.RandomState(1000 + seed)
    while True:
        ncols, nrows = int(rs.randint(1, 201)), int(rs.randint(1, 151))
        tiles_x, tiles_y = int(rs.randint(1, min(64, ncols) + 1)), int(rs.randint(1, min(64, nrows) + 1))
        if equalisable(ncols, nrows, tiles_x, tiles_y):
            break
    clip_q8 = int(rs.choice([0, 1, 256, 768, 10240, 1 << 20, int(rs.randint(1, 1 << 20))]))
    pitch = ncols + int(rs.choice([0, 0, 1, 13, 16]))
    kind = int(rs.randint(0, 3))
    frame = (random_frame(ncols, nrows, seed), two_bin_frame(ncols, nrows, seed), rs.randint(0, 256, (nrows, ncols)).astype(np.uint8))[kind]
    return frame, tiles_x, tiles_y, clip_q8, pitch
