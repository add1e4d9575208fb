"""What the TUM-RGBD fixtures' generator (make_golden_tum.py) and the tests share: an independent numpy
restatement of the undistortion contract (include/nslam.h nslam_undistort_u8) and the synthetic sequence.

Nothing here imports the product or the reference.  The restatement is written apart from the product's host
twin (datasets.undistort_u8) on purpose: per channel, floor division and modulo where the product shifts and
masks, so the two only agree when both follow the contract.  It is a restatement of cv2.undistort's documented
defaults (new camera matrix K, bilinear, constant zero border, 1/32-pixel positions); parity with OpenCV itself
is unpinned (library absent).
"""
import io

import numpy as np

# configs/TUM_RGBD/freiburg1_*.yaml: the intrinsics and the five coefficients (k1, k2, p1, p2, k3)
FREIBURG1 = {"fx": 517.3, "fy": 516.5, "cx": 318.6, "cy": 255.3}
FREIBURG1_DIST = [0.2624, -0.9531, -0.0054, 0.0026, 1.1633]


def intrinsics(scale=1.0):
    """freiburg1's (fx, fy, cx, cy) × scale (a smaller image of the same lens)."""
    return tuple(FREIBURG1[k] * scale for k in ("fx", "fy", "cx", "cy"))


def undistort_map(H, W, fx, fy, cx, cy, dist):
    """The float64 source position (map_x, map_y), in pixels, of every destination pixel."""
    k1, k2, p1, p2, k3 = (float(d) for d in dist)
    map_x = np.empty((H, W), dtype=np.float64)
    map_y = np.empty((H, W), dtype=np.float64)
    u = np.arange(W, dtype=np.float64)
    for v in range(H):
        x = (u - cx) / fx
        y = (np.float64(v) - cy) / fy
        r2 = x * x + y * y
        rad = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2
        xd = x * rad + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
        yd = y * rad + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
        map_x[v] = xd * fx + cx
        map_y[v] = yd * fy + cy
    return map_x, map_y


def near_half(map_x, map_y, tol=1e-6):
    """Pixels whose 32·map_x or 32·map_y lies within tol of a half-integer: there a last-bit difference in the
    float64 map may round to the other 1/32 cell."""
    def frac_half(m):
        t = m * 32.0
        return np.abs(t - np.floor(t) - 0.5)
    return (frac_half(map_x) <= tol) | (frac_half(map_y) <= tol)


def undistort_u8(src, fx, fy, cx, cy, dist):
    """dst = cv2.undistort(src, K, dist) by the contract, for a uint8 image [H, W] or [H, W, C]."""
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim in (2, 3)
    H, W = src.shape[:2]
    map_x, map_y = undistort_map(H, W, fx, fy, cx, cy, dist)
    lim = 2.0 ** 30
    X = np.rint(np.clip(np.where(np.isnan(map_x), -lim, map_x * 32.0), -lim, lim)).astype(np.int64)
    Y = np.rint(np.clip(np.where(np.isnan(map_y), -lim, map_y * 32.0), -lim, lim)).astype(np.int64)
    x0, ax = np.floor_divide(X, 32), np.mod(X, 32)
    y0, ay = np.floor_divide(Y, 32), np.mod(Y, 32)
    planes = src.reshape(H, W, -1)
    out = np.zeros(planes.shape, dtype=np.uint8)
    for c in range(planes.shape[2]):
        pad = np.zeros((H + 2, W + 2), dtype=np.int64)  # the zero border, one pixel wide
        pad[1:-1, 1:-1] = planes[:, :, c]

        def S(xx, yy):
            inside = (xx >= -1) & (xx <= W) & (yy >= -1) & (yy <= H)
            return np.where(inside, pad[np.clip(yy, -1, H) + 1, np.clip(xx, -1, W) + 1], 0)

        acc = ((32 - ax) * (32 - ay) * S(x0, y0) + ax * (32 - ay) * S(x0 + 1, y0)
               + (32 - ax) * ay * S(x0, y0 + 1) + ax * ay * S(x0 + 1, y0 + 1) + 512)
        out[:, :, c] = np.floor_divide(acc, 1024)
    return out.reshape(src.shape)


def taps_outside(H, W, fx, fy, cx, cy, dist):
    """Number of destination pixels with at least one of the four taps outside the image."""
    map_x, map_y = undistort_map(H, W, fx, fy, cx, cy, dist)
    x0 = np.floor(np.rint(map_x * 32.0) / 32.0)
    y0 = np.floor(np.rint(map_y * 32.0) / 32.0)
    return int(((x0 < 0) | (x0 + 1 >= W) | (y0 < 0) | (y0 + 1 >= H)).sum())


def random_u8(H, W, C, seed):
    """Seeded random bytes: every tap matters."""
    return np.random.default_rng(seed).integers(0, 256, (H, W, C), dtype=np.uint8)


# ------------------------------------------------------------------------------------------------
# the synthetic TUM-RGBD folder (48×64)
# ------------------------------------------------------------------------------------------------
SEQ_H, SEQ_W = 48, 64
SEQ_SCALE = 1.5
SEQ_CAM = dict(zip(("fx", "fy", "cx", "cy"), intrinsics(0.1)), H=SEQ_H, W=SEQ_W, png_depth_scale=5000.0,
               crop_size=[40, 52], crop_edge=2, distortion=FREIBURG1_DIST)

# colour stamps: 10.00 kept; 10.02 closer than 1/32 s to it (thinned out); 10.10 kept; 10.30 has no depth
# within 0.08 s; 10.50 has no pose within 0.08 s; 12.00 lies exactly between two depth stamps (binary
# fractions: |Δt| = 0.0625 to both, the first wins); 12.20 kept
SEQ_COLOR_T = ["10.0000", "10.0200", "10.1000", "10.3000", "10.5000", "12.0000", "12.2000"]
SEQ_DEPTH_T = ["10.0100", "10.1100", "10.5000", "11.9375", "12.0625", "12.2100"]
SEQ_POSE_T = ["10.0050", "10.0300", "10.1100", "10.3000", "10.7000", "12.0100", "12.1900"]
SEQ_KEPT = [(0, 0, 0), (2, 1, 2), (5, 3, 5), (6, 5, 6)]  # (colour, depth, pose) rows the loader must choose


def _png(arr):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(arr).save(b, format="PNG")
    return b.getvalue()


def tum_sequence(seed=7):
    """{relative path: bytes} of the folder: rgb.txt, depth.txt, groundtruth.txt ('#' header lines in each),
    rgb/<t>.png (8-bit colour, lossless) and depth/<t>.png (16-bit)."""
    rng = np.random.default_rng(seed)
    files = {}
    yy, xx = np.mgrid[0:SEQ_H, 0:SEQ_W]
    rgb = ["# color images", "# file: 'synthetic.bag'", "# timestamp filename"]
    for t in SEQ_COLOR_T:
        ph = rng.uniform(0, 6, 3)
        img = np.stack([127 + 120 * np.sin(xx / (2 + k) + yy / (3 + k) + ph[k]) for k in range(3)], -1)
        img = np.clip(img + rng.integers(-6, 7, img.shape), 0, 255).astype(np.uint8)
        files[f"rgb/{t}.png"] = _png(img)
        rgb.append(f"{t} rgb/{t}.png")
    dep = ["# depth maps", "# file: 'synthetic.bag'", "# timestamp filename"]
    for t in SEQ_DEPTH_T:
        d = rng.integers(0, 30000, (SEQ_H, SEQ_W)).astype(np.uint16)
        d[rng.random((SEQ_H, SEQ_W)) < 0.05] = 0
        files[f"depth/{t}.png"] = _png(d)
        dep.append(f"{t} depth/{t}.png")
    gt = ["# ground truth trajectory", "# file: 'synthetic.bag'", "# timestamp tx ty tz qx qy qz qw"]
    for t in SEQ_POSE_T:
        q = rng.normal(size=4)
        q = np.round(q / np.linalg.norm(q), 4)  # four decimals, as the dataset's files: not quite unit length
        tr = np.round(rng.normal(size=3), 4)
        gt.append(" ".join([t] + [f"{v:.4f}" for v in tr] + [f"{v:.4f}" for v in q]))
    files["rgb.txt"] = ("\n".join(rgb) + "\n").encode()
    files["depth.txt"] = ("\n".join(dep) + "\n").encode()
    files["groundtruth.txt"] = ("\n".join(gt) + "\n").encode()
    return files
