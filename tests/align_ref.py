"""Independent restatements for the alignment tests (tests/test_align_host.py, tests/test_gpu_align.py), written from the papers
and not from tf_face_toolbox_amd/preprocessing.py: Umeyama's least-squares similarity by SVD with the determinant correction
(Umeyama 1991, eq. 40-43), a direct float64 bilinear warp with zero fill, and a generator of synthetic dot images."""
import os

import numpy as np

IMG = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'images')

# ArcFace's norm_crop template for 112 x 112, typed in again here
TEMPLATE_112 = np.array([[38.2946, 51.6963], [73.5318, 51.5014], [56.0252, 71.7366], [41.5493, 92.3655], [70.7299, 92.2041]])


def umeyama(src, dst):
    """float64 [2, 3] similarity (rotation, uniform scale, translation; no reflection) minimising sum |c R src + t - dst|^2"""
    src = np.asarray(src, dtype=np.float64).reshape(-1, 2)
    dst = np.asarray(dst, dtype=np.float64).reshape(-1, 2)
    n = src.shape[0]
    ms, md = src.mean(0), dst.mean(0)
    p, q = src - ms, dst - md
    cov = q.T @ p / n
    u, d, vt = np.linalg.svd(cov)
    s = np.ones(2)
    if np.linalg.det(cov) < 0:
        s[-1] = -1
    r = u @ np.diag(s) @ vt
    c = (d * s).sum() / ((p * p).sum() / n)
    m = c * r
    return np.concatenate([m, (md - m @ ms)[:, None]], 1)


def similarity(angle_deg, scale, tx=0.0, ty=0.0):
    a = np.deg2rad(angle_deg)
    return np.array([[scale * np.cos(a), -scale * np.sin(a), tx], [scale * np.sin(a), scale * np.cos(a), ty]])


def apply(m, pts):
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 2)
    return pts @ m[:, :2].T + m[:, 2]


def invert(m):
    inv = np.linalg.inv(m[:, :2])
    return np.concatenate([inv, (-inv @ m[:, 2])[:, None]], 1)


def warp64(image, inv, out_h, out_w):
    """out[y, x] = bilinear sample of `image` (float HWC) at inv @ (x, y, 1), float64 throughout, zero outside the image"""
    image = np.asarray(image, dtype=np.float64)
    h, w = image.shape[:2]
    out = np.zeros((out_h, out_w, image.shape[2]))
    for y in range(out_h):
        for x in range(out_w):
            sx = inv[0, 0] * x + inv[0, 1] * y + inv[0, 2]
            sy = inv[1, 0] * x + inv[1, 1] * y + inv[1, 2]
            fx, fy = int(np.floor(sx)), int(np.floor(sy))
            for yy, wy in ((fy, fy + 1 - sy), (fy + 1, sy - fy)):
                for xx, wx in ((fx, fx + 1 - sx), (fx + 1, sx - fx)):
                    if 0 <= yy < h and 0 <= xx < w:
                        out[y, x] += wy * wx * image[yy, xx]
    return out


def dot_image(h, w, points, channels=3, half=2, background=0):
    """uint8 [h, w, channels]: `background` everywhere, a (2 half + 1)^2 block of 255 centred on each rounded (x, y) point"""
    img = np.full((h, w, channels), background, dtype=np.uint8)
    for x, y in np.asarray(points, dtype=np.float64).reshape(-1, 2):
        cx, cy = int(round(x)), int(round(y))
        img[max(cy - half, 0):cy + half + 1, max(cx - half, 0):cx + half + 1] = 255
    return img


def centroid(plane, x, y, half=3):
    """intensity centroid (x, y) of the (2 half + 1)^2 window of a 2-D plane around the rounded point"""
    cx, cy = int(round(x)), int(round(y))
    y0, x0 = max(cy - half, 0), max(cx - half, 0)
    win = np.asarray(plane, dtype=np.float64)[y0:cy + half + 1, x0:cx + half + 1]
    ys, xs = np.mgrid[y0:y0 + win.shape[0], x0:x0 + win.shape[1]]
    tot = win.sum()
    return (win * xs).sum() / tot, (win * ys).sum() / tot


def golden_lists(tmp_path):
    """tests/golden/images/list.txt and landmarks.txt with absolute image paths, written under tmp_path:
    (list path, landmark list path, [image paths], [labels], float32 [n, 10] landmarks)"""
    paths, labels, marks = [], [], {}
    for ln in open(os.path.join(IMG, 'list.txt')):
        if ln.split():
            paths.append(os.path.join(IMG, ln.split()[0]))
            labels.append(int(ln.split()[1]))
    for ln in open(os.path.join(IMG, 'landmarks.txt')):
        if ln.split():
            marks[os.path.join(IMG, ln.split()[0])] = ln.split()[1:]
    lst, lml = tmp_path / 'list_abs.txt', tmp_path / 'landmarks_abs.txt'
    lst.write_text(''.join('%s %d\n' % (p, lab) for p, lab in zip(paths, labels)))
    lml.write_text(''.join('%s %s\n' % (p, ' '.join(marks[p])) for p in paths))
    lm = np.asarray([[float(v) for v in marks[p]] for p in paths], dtype=np.float32)
    return str(lst), str(lml), paths, labels, lm
