"""numpy reference for radnerf/prepare.py (shared helper, no test): the data flow of the reference's data_utils/process.py tasks 5 and 6
in ITS index style -- brute-force distances where it asks a k-d tree, lexsort / unique / fancy indexing for the in-paints -- so that it
shares nothing with the kernels' per-column form.  Two places follow the stated departures instead of numpy's wrap-around: in-paint
rows above row 0 are dropped, and a top at row 0 has no head above.  The blur is the stated integer 5 x 5 with reflect-101 edges.

Also the synthetic label maps the tests use.
"""
import numpy as np

OTHER, HEAD, NECK, TORSO, BACKGROUND = 0, 1, 2, 3, 4
FAR = 1 << 30
BLUR = np.array([48, 53, 54, 53, 48], dtype=np.int64)


def squared_distances(label):
    """int64 [H,W]: squared distance of every pixel to the nearest pixel that is not BACKGROUND, all pairs; FAR without one."""
    h, w = label.shape
    all_xys = np.mgrid[0:h, 0:w].reshape(2, -1).transpose()
    fg_xys = np.stack(np.nonzero(label != BACKGROUND)).transpose(1, 0)
    if fg_xys.shape[0] == 0:
        return np.full((h, w), FAR, dtype=np.int64)
    out = np.empty(h * w, dtype=np.int64)
    for at in range(0, h * w, 512):
        d = all_xys[at:at + 512, None, :].astype(np.int64) - fg_xys[None].astype(np.int64)
        out[at:at + 512] = (d * d).sum(-1).min(1)
    return out.reshape(h, w)


def plate_accumulate(frames, labels):
    """(best_d2 int64 [H,W], best_id [H,W], plate uint8 [H,W,3]): process.py:78-104 with the colour kept for EVERY pixel."""
    f, h, w = labels.shape
    distss = np.stack([squared_distances(l).reshape(-1) for l in labels])
    max_dist = np.max(distss, 0)
    max_id = np.argmax(distss, 0)
    imgs = frames.reshape(f, h * w, 3)
    plate = imgs[max_id, np.arange(h * w), :]
    return max_dist.reshape(h, w), max_id.reshape(h, w), plate.reshape(h, w, 3)


def plate_fill(best_d2, plate, thresh_d2=25):
    """(filled plate, source [H,W,2], n_sure): process.py:106-113.  np.nonzero lists the sure pixels by row, then column, and argmin
    takes the first minimum: the smallest source row, then the smallest source column."""
    bc_pixs = best_d2 > thresh_d2
    bg_xys = np.stack(np.nonzero(~bc_pixs)).transpose()
    fg_xys = np.stack(np.nonzero(bc_pixs)).transpose()
    out = plate.copy()
    h, w = best_d2.shape
    source = np.mgrid[0:h, 0:w].transpose(1, 2, 0).copy()
    if fg_xys.shape[0] == 0 or bg_xys.shape[0] == 0:
        return out, source, int(fg_xys.shape[0])
    d = bg_xys[:, None, :].astype(np.int64) - fg_xys[None].astype(np.int64)
    indices = (d * d).sum(-1).argmin(1)
    bg_fg_xys = fg_xys[indices]
    out[bg_xys[:, 0], bg_xys[:, 1], :] = plate[bg_fg_xys[:, 0], bg_fg_xys[:, 1], :]
    source[bg_xys[:, 0], bg_xys[:, 1]] = bg_fg_xys
    return out, source, int(fg_xys.shape[0])


def background_plate(frames, labels, thresh_d2=25):
    best_d2, _, plate = plate_accumulate(frames, labels)
    return plate_fill(best_d2, plate, thresh_d2)[0]


def dilate_rows(mask, r=3):
    """binary_dilation with a 3 x 1 vertical structure, r iterations: any of rows y - r .. y + r, zeros outside."""
    h = mask.shape[0]
    out = np.zeros_like(mask)
    for d in range(-r, r + 1):
        out[max(0, d):h + min(0, d)] |= mask[max(0, -d):h - max(0, d)]
    return out


def integer_blur(img):
    """(sum of w_i w_j p + 32768) >> 16 over 5 x 5, reflect-101."""
    h, w = img.shape[:2]
    pad = np.pad(img.astype(np.int64), ((2, 2), (2, 2), (0, 0)), mode="reflect")
    acc = np.zeros(img.shape, dtype=np.int64)
    for i in range(5):
        for j in range(5):
            acc += BLUR[i] * BLUR[j] * pad[i:i + h, j:j + w]
    return ((acc + 32768) >> 16).astype(np.uint8)


def _inpaint(image, gt_image, head_part, part, L, push_down):
    """process.py:152-181 / 186-223 for one part mask; returns the in-paint mask (all False when nothing is painted)."""
    coords = np.stack(np.nonzero(part), axis=-1)
    inds = np.lexsort((coords[:, 0], coords[:, 1]))
    coords = coords[inds]
    u, uid, ucnt = np.unique(coords[:, 1], return_index=True, return_counts=True)
    top = coords[uid]
    up = top.copy() - np.array([1, 0])
    mask = (top[:, 0] >= 1) & head_part[tuple(up.T)] if top.shape[0] else np.zeros(0, dtype=bool)     # departure: row 0 has no head above
    out = np.zeros(image.shape[:2], dtype=bool)
    if not mask.any():
        return out
    top = top[mask]
    if push_down:
        offset_down = np.minimum(ucnt[mask] - 1, push_down)
        top = top + np.stack([offset_down, np.zeros_like(offset_down)], axis=-1)
    colors = gt_image[tuple(top.T)]
    inpaint_coords = top[None].repeat(L, 0)
    inpaint_coords = inpaint_coords + np.stack([-np.arange(L), np.zeros(L, dtype=np.int64)], axis=-1)[:, None]
    inpaint_coords = inpaint_coords.reshape(-1, 2)
    darken_scaler = 0.98 ** np.arange(L).reshape(L, 1, 1)
    inpaint_colors = (colors[None].repeat(L, 0) * darken_scaler).reshape(-1, 3)
    keep = inpaint_coords[:, 0] >= 0                                                                   # departure: rows above 0 are dropped
    inpaint_coords, inpaint_colors = inpaint_coords[keep], inpaint_colors[keep]
    image[tuple(inpaint_coords.T)] = inpaint_colors.astype(np.uint8)                                   # float64 -> uint8 truncates
    out[tuple(inpaint_coords.T)] = True
    return out


def layers(frame, label, plate):
    """(gt uint8 [H,W,3], torso uint8 [H,W,4]) of one frame: process.py:131-237."""
    head_part, neck_part, torso_part, bg_part = (label == v for v in (HEAD, NECK, TORSO, BACKGROUND))
    gt_image = frame.copy()
    gt_image[bg_part] = plate[bg_part]
    torso_image = gt_image.copy()
    torso_image[head_part] = plate[head_part]
    inpaint_torso_mask = _inpaint(torso_image, gt_image, head_part, torso_part, 8 + 1, 0)
    neck_part = dilate_rows(neck_part, 3)
    inpaint_mask = _inpaint(torso_image, gt_image, head_part, neck_part, 48 + 4 + 1, 4)
    blur_img = integer_blur(torso_image)
    torso_image[inpaint_mask] = blur_img[inpaint_mask]
    mask = neck_part | torso_part | inpaint_mask | inpaint_torso_mask
    torso_image[~mask] = 0
    alpha = np.where(mask, 255, 0).astype(np.uint8)
    return gt_image, np.concatenate([torso_image, alpha[..., None]], axis=-1)


def layers_batch(frames, labels, plate):
    out = [layers(f, l, plate) for f, l in zip(frames, labels)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


# ----------------------------------------------------------------------------------------------------------------- inputs
def moving_blob(F, H, W, rng, other=True):
    """Labels: background with a foreground box that moves from frame to frame, and a few stray pixels of every class."""
    labels = np.full((F, H, W), BACKGROUND, dtype=np.uint8)
    bh, bw = max(1, H // 3), max(1, W // 3)
    for f in range(F):
        y0, x0 = rng.integers(0, max(1, H - bh)), rng.integers(0, max(1, W - bw))
        labels[f, y0:y0 + bh, x0:x0 + bw] = rng.integers(0, 4, (min(H - y0, bh), min(W - x0, bw)))
        if other:
            stray = rng.random((H, W)) < 0.01
            labels[f][stray] = rng.integers(0, 4, int(stray.sum()))
    return labels


EDGE_SHAPES = [(7, 1), (7, 63), (7, 64), (7, 65), (1, 9), (1, 1), (3, 300)]       # the wave width, one row, one pixel, two workgroups a row


def plate_cases():
    """name -> (frames uint8 [F,H,W,3], labels uint8 [F,H,W]): every plate input of the tests."""
    out = {}
    rng = np.random.default_rng(505)
    out["40x56"] = (rng.integers(0, 256, (5, 40, 56, 3), dtype=np.uint8), moving_blob(5, 40, 56, rng))
    for H, W in EDGE_SHAPES:
        rng = np.random.default_rng(H * 1000 + W)
        frames = rng.integers(0, 256, (3, H, W, 3), dtype=np.uint8)
        labels = moving_blob(3, H, W, rng, other=False)
        labels[0, H - 1, W - 1] = NECK
        labels[1, 0, 0] = BACKGROUND
        out[f"{H}x{W}"] = (frames, labels)
    rng = np.random.default_rng(77)
    frames = rng.integers(0, 256, (3, 9, 70, 3), dtype=np.uint8)
    labels = np.full((3, 9, 70), BACKGROUND, dtype=np.uint8)
    labels[0, 8, 69] = OTHER                          # one foreground pixel, in a corner
    labels[2, 0, 0] = HEAD                            # frame 1 has none: it is all background, at 2^30
    out["empty_and_corner"] = (frames, labels)
    frames, labels = out["40x56"]
    twice = np.concatenate([frames[:1], frames[:1], frames[1:2]])
    twice[1] = 255 - twice[1]                         # the same labels, other colours: the plate shows which frame was taken
    out["identical_frames"] = (twice, np.concatenate([labels[:1], labels[:1], labels[1:2]]))
    return out


def portrait_labels(h, w, rng, neck=True, neck_top=None, torso_top=None, holes=0.02, jag=3):
    """A head over a neck over a torso on background, with jagged neck and torso tops and a share of OTHER holes.
    neck_top / torso_top move the (mean) top rows; neck=False leaves the neck out (the head then sits on the torso)."""
    label = np.full((h, w), BACKGROUND, dtype=np.uint8)
    cols = np.arange(w)
    nt = (h * 4 // 10 if neck_top is None else neck_top) + rng.integers(0, jag + 1, w)
    tt = (h * 6 // 10 if torso_top is None else torso_top) + rng.integers(0, jag + 1, w)
    rows = np.arange(h)[:, None]
    head = (rows >= h // 10) & (rows < np.maximum(nt, 0)[None]) & (np.abs(cols - w // 2) < w // 4)[None]
    neck_m = (rows >= nt[None]) & (rows < tt[None]) & (np.abs(cols - w // 2) < w // 8)[None]
    torso = (rows >= tt[None]) & (np.abs(cols - w // 2) < (w * 3) // 8)[None]
    label[head] = HEAD
    if neck:
        label[neck_m] = NECK
    else:
        label[neck_m] = HEAD
    label[torso] = TORSO
    if holes:
        label[rng.random((h, w)) < holes] = OTHER
    return label


def parsing_from_labels(label):
    """The RGB parsing image of a label map; OTHER becomes a colour that is none of the four."""
    table = np.array([(10, 20, 30), (0, 0, 255), (0, 255, 0), (255, 0, 0), (255, 255, 255)], dtype=np.uint8)
    return table[label]
