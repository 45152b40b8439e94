"""The remap ingest stage's rule (include/klt_gpu.h, "Remap ingest stage") restated in numpy, the maps the tests run
it under and seeded draws.  Integer arithmetic only: the device must equal `remap` byte for byte."""
import numpy as np

INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def remap(frame, mx, my):
    """the rule on a 2-D uint8 array under two int32 arrays of its shape (source positions in 1/256 px) -> uint8 array of that shape"""
    frame, mx, my = np.asarray(frame), np.asarray(mx), np.asarray(my)
    assert frame.dtype == np.uint8 and frame.ndim == 2 and mx.shape == frame.shape == my.shape
    assert mx.dtype == np.int32 and my.dtype == np.int32
    nrows, ncols = frame.shape
    X = np.clip(mx.astype(np.int64), 0, (ncols - 1) * 256)
    Y = np.clip(my.astype(np.int64), 0, (nrows - 1) * 256)
    x0, fx, y0, fy = X >> 8, X & 255, Y >> 8, Y & 255
    x1, y1 = np.minimum(x0 + 1, ncols - 1), np.minimum(y0 + 1, nrows - 1)
    p = frame.astype(np.int64)
    s = ((256 - fx) * (256 - fy) * p[y0, x0] + fx * (256 - fy) * p[y0, x1] + (256 - fx) * fy * p[y1, x0] + fx * fy * p[y1, x1] + 32768)
    assert s.max() < 2 ** 32
    return (s >> 16).astype(np.uint8)


# -------------------------------------------------------------------------------------------------------------------------- maps
def _grid(ncols, nrows):
    y, x = np.mgrid[0:nrows, 0:ncols]
    return x.astype(np.float64), y.astype(np.float64)


def _entries(x, y):
    """float source positions in px -> the two int32 planes"""
    return tuple(np.clip(np.rint(256.0 * a), INT32_MIN, INT32_MAX).astype(np.int32) for a in (x, y))


def identity_map(ncols, nrows):
    return _entries(*_grid(ncols, nrows))


def shift_map(ncols, nrows, dx=2.37, dy=-1.61):
    """destination (x, y) reads source (x + dx, y + dy): a fractional shift, replicated edges on two sides"""
    x, y = _grid(ncols, nrows)
    return _entries(x + dx, y + dy)


def rotation_map(ncols, nrows, degrees=17.0):
    x, y = _grid(ncols, nrows)
    cx, cy, a = (ncols - 1) / 2.0, (nrows - 1) / 2.0, np.deg2rad(degrees)
    return _entries(cx + np.cos(a) * (x - cx) - np.sin(a) * (y - cy), cy + np.sin(a) * (x - cx) + np.cos(a) * (y - cy))


def barrel_map(ncols, nrows, k1=-0.25, k2=0.05):
    """undistortion of a barrel lens: the forward radial model about the centre, focal length the half diagonal"""
    x, y = _grid(ncols, nrows)
    cx, cy = (ncols - 1) / 2.0, (nrows - 1) / 2.0
    f = max(1.0, np.hypot(ncols, nrows) / 2.0)
    u, v = (x - cx) / f, (y - cy) / f
    r2 = u * u + v * v
    radial = 1.0 + r2 * (k1 + r2 * k2)
    return _entries(cx + f * u * radial, cy + f * v * radial)


def transpose_map(ncols, nrows):
    """neighbouring destination pixels of a row read neighbouring ROWS of the source: the worst source locality.  Destination (x, y)
    reads source (y scaled to the width, x scaled to the height), a quarter pixel off the centres"""
    x, y = _grid(ncols, nrows)
    sx = y * ((ncols - 1) / max(1.0, nrows - 1.0)) + 0.25
    sy = x * ((nrows - 1) / max(1.0, ncols - 1.0)) + 0.25
    return _entries(sx, sy)


def wild_map(ncols, nrows, seed=11):
    """uniform int32 -- negatives, values far outside the frame -- a share of entries inside the frame, and the extremes"""
    rs = np.random.RandomState(seed)
    out = []
    for n in (ncols, nrows):
        m = rs.randint(INT32_MIN, INT32_MAX + 1, (nrows, ncols), dtype=np.int64)
        inside = rs.rand(nrows, ncols) < 0.5
        m[inside] = rs.randint(-512, n * 256 + 512, int(inside.sum()))
        flat = m.ravel()
        picks = rs.randint(0, flat.size, 4)
        flat[picks[0]], flat[picks[1]] = INT32_MIN, INT32_MAX
        flat[picks[2]], flat[picks[3]] = (n - 1) * 256, (n - 1) * 256 + 1
        out.append(m.astype(np.int32))
    return out[0], out[1]


MAPS = {"identity": identity_map, "shift": shift_map, "rotation": rotation_map, "barrel": barrel_map, "transpose": transpose_map, "wild": wild_map}


# ------------------------------------------------------------------------------------------------------------------------ frames
def random_frame(ncols, nrows, seed):
    return np.random.RandomState(seed).randint(0, 256, (nrows, ncols)).astype(np.uint8)


def constant_frame(ncols, nrows, value=77):
    return np.full((nrows, ncols), value, np.uint8)


def two_level_frame(ncols, nrows, seed=5):
    """0 and 255 only: every interpolation weight shows in the output"""
    return np.where(np.random.RandomState(seed).rand(nrows, ncols) < 0.5, 0, 255).astype(np.uint8)


def textured_frame(ncols, nrows, seed):
    """smooth texture with noise: what a selection finds corners in"""
    yy, xx = np.mgrid[0:nrows, 0:ncols]
    rs = np.random.RandomState(seed)
    f = 120 + 60 * np.sin(xx / 7.0 + seed) * np.cos(yy / 11.0) + 40 * np.sin((xx + 2 * yy) / 5.0) + rs.normal(0, 8, (nrows, ncols))
    return np.clip(f, 0, 255).astype(np.uint8)


def trial(seed):
    """one seeded draw: (frame, (mx, my), pitch, name of the map) with a frame up to 200 x 150"""
    rs = np.random.RandomState(2000 + seed)
    ncols, nrows = int(rs.randint(1, 201)), int(rs.randint(1, 151))
    name = sorted(MAPS)[int(rs.randint(0, len(MAPS)))]
    if name == "shift":
        m = shift_map(ncols, nrows, float(rs.uniform(-9, 9)), float(rs.uniform(-9, 9)))
    elif name == "rotation":
        m = rotation_map(ncols, nrows, float(rs.uniform(-180, 180)))
    elif name == "wild":
        m = wild_map(ncols, nrows, seed)
    else:
        m = MAPS[name](ncols, nrows)
    pitch = ncols + int(rs.choice([0, 0, 1, 13, 16]))
    kind = int(rs.randint(0, 3))
    frame = (random_frame(ncols, nrows, seed), two_level_frame(ncols, nrows, seed), textured_frame(ncols, nrows, seed))[kind]
    return frame, m, pitch, name
