"""Third-party pieces and data of the segmentation input-pipeline tests (tests/golden/seg_data*.npz, scripts/make_golden_seg_data.py).

The reference's loader (utils/segment/dataloaders.py) turns polygons into masks with functions that are NOT in its tree:
`cv2.fillPoly` / `cv2.resize` (opencv-python) and `polygon2mask` / `polygons2masks` / `polygons2masks_overlap` (ultralytics.data.utils).
Neither package is installed where the golden files are written, so they are restated here from the published sources and are PARITY
UNPINNED BY NECESSITY, like oracle/thirdparty.py:

  fill_poly        OpenCV modules/imgproc/src/drawing.cpp: fillPoly -> CollectPolyEdges (one contour, LINE_8, shift 0; the revision that
                   draws every edge with Line(), clips the edge with clipLine() when an end point lies outside the image and otherwise adds
                   XY_ONE / 2 to both x) -> FillEdgeCollection (edges sorted by (y0, x, dx), active list kept sorted by x, spans between
                   consecutive pairs, x1 = x >> XY_SHIFT on both ends for a non-antialiased line type).  Line() = LineIterator(8-connected,
                   left to right) after clipLine().
  polygon2mask...  ultralytics/data/utils.py.  NOTE polygons2masks_overlap adds uint8 planes: with more than 128 overlapping instances
                   `masks + mask` wraps before the clip.  The kernel's contract (1 + rank of the last covering instance) is what the loop
                   computes whenever it does not wrap; the tests stay below 129 or above 255 instances (int32 there) per image.

`check_fill_geometry` is the check that does NOT rest on these restatements (exact integer geometry), run on the restatement and on the
kernel alike.  `polygon_dataset` is the seeded synthetic polygon dataset of the golden files and tests.
"""
import numpy as np

XY_SHIFT = 16
XY_ONE = 1 << XY_SHIFT


# ---- cv2.clipLine / Line / fillPoly -----------------------------------------------------------------------------------------------------
def _trunc_div(a, b):
    """(int64)((double)a_times / b): the callers pass the double product; C truncation toward zero."""
    return int(a / b)


def clip_line(w, h, p1, p2):
    """cv::clipLine(Size2l, Point2l&, Point2l&): returns (inside, p1, p2)."""
    x1, y1 = p1
    x2, y2 = p2
    right, bottom = w - 1, h - 1
    if w <= 0 or h <= 0:
        return False, (x1, y1), (x2, y2)
    c1 = (x1 < 0) + (x1 > right) * 2 + (y1 < 0) * 4 + (y1 > bottom) * 8
    c2 = (x2 < 0) + (x2 > right) * 2 + (y2 < 0) * 4 + (y2 > bottom) * 8
    if (c1 & c2) == 0 and (c1 | c2) != 0:
        if c1 & 12:
            a = 0 if c1 < 8 else bottom
            x1 += _trunc_div(float(a - y1) * (x2 - x1), (y2 - y1))
            y1 = a
            c1 = (x1 < 0) + (x1 > right) * 2
        if c2 & 12:
            a = 0 if c2 < 8 else bottom
            x2 += _trunc_div(float(a - y2) * (x2 - x1), (y2 - y1))
            y2 = a
            c2 = (x2 < 0) + (x2 > right) * 2
        if (c1 & c2) == 0 and (c1 | c2) != 0:
            if c1:
                a = 0 if c1 == 1 else right
                y1 += _trunc_div(float(a - x1) * (y2 - y1), (x2 - x1))
                x1 = a
                c1 = 0
            if c2:
                a = 0 if c2 == 1 else right
                y2 += _trunc_div(float(a - x2) * (y2 - y1), (x2 - x1))
                x2 = a
                c2 = 0
    return (c1 | c2) == 0, (x1, y1), (x2, y2)


def draw_line(img, p1, p2, color):
    """Line(img, pt1, pt2, color, 8): LineIterator(img, pt1, pt2, 8, leftToRight = true)."""
    h, w = img.shape
    if not (0 <= p1[0] < w and 0 <= p2[0] < w and 0 <= p1[1] < h and 0 <= p2[1] < h):
        ok, p1, p2 = clip_line(w, h, p1, p2)
        if not ok:
            return
    dx, dy = p2[0] - p1[0], p2[1] - p1[1]
    x, y = p1
    sx = sy = 1
    if dx < 0:
        dx, dy = -dx, -dy
        x, y = p2
    if dy < 0:
        dy, sy = -dy, -1
    vert = dy > dx
    if vert:
        dx, dy = dy, dx
    err = dx - (dy + dy)
    plus_delta, minus_delta = dx + dx, -(dy + dy)
    for _ in range(dx + 1):
        img[y, x] = color
        neg = err < 0
        err += minus_delta + (plus_delta if neg else 0)
        if vert:
            y += sy
            x += sx if neg else 0
        else:
            x += sx
            y += sy if neg else 0


def _collect_poly_edges(img, pts, color):
    h, w = img.shape
    edges = []
    n = len(pts)
    x0, y0 = int(pts[n - 1][0]) << XY_SHIFT, int(pts[n - 1][1])
    for i in range(n):
        x1, y1 = int(pts[i][0]) << XY_SHIFT, int(pts[i][1])
        t0 = ((x0 + (XY_ONE >> 1)) >> XY_SHIFT, y0)
        t1 = ((x1 + (XY_ONE >> 1)) >> XY_SHIFT, y1)
        draw_line(img, t0, t1, color)
        c0x, c0y, c1x, c1y = x0, y0, x1, y1
        if not (0 <= t0[0] < w and 0 <= t1[0] < w and 0 <= t0[1] < h and 0 <= t1[1] < h):
            _, t0, t1 = clip_line(w, h, t0, t1)
            if t0[1] != t1[1]:
                c0y, c1y = t0[1], t1[1]
                c0x, c1x = t0[0] << XY_SHIFT, t1[0] << XY_SHIFT
        else:
            c0x += XY_ONE >> 1
            c1x += XY_ONE >> 1
        if y0 != y1:
            num, den = c1x - c0x, c1y - c0y
            dx = abs(num) // abs(den) * (1 if (num < 0) == (den < 0) else -1)   # C++ integer division truncates toward zero
            if y0 < y1:
                edges.append([y0, y1, c0x + (y0 - c0y) * dx, dx])
            else:
                edges.append([y1, y0, c1x + (y1 - c1y) * dx, dx])
        x0, y0 = x1, y1
    return edges


def _fill_edge_collection(img, edges, color):
    """FillEdgeCollection for a non-antialiased line type (delta = 0).  An edge is [y0, y1, x, dx]."""
    h, w = img.shape
    total = len(edges)
    if total < 2:
        return
    y_min, y_max, x_min, x_max = min(e[0] for e in edges), max(e[1] for e in edges), (1 << 63) - 1, -1
    for e in edges:
        x1 = e[2] + (e[1] - e[0]) * e[3]
        x_min, x_max = min(x_min, e[2], x1), max(x_max, e[2], x1)
    if y_max < 0 or y_min >= h or x_max < 0 or x_min >= (w << XY_SHIFT):
        return
    edges.sort(key=lambda e: (e[0], e[2], e[3]))
    active, i = [], 0
    y_max = min(y_max, h)
    for y in range(edges[0][0], y_max):
        merged, li, draw, cur = [], 0, 0, None
        while li < len(active) or (i < total and edges[i][0] == y):
            if li < len(active) and active[li][1] == y:      # exclude edge if y reaches its lower point
                li += 1
                continue
            keep = cur
            if li < len(active) and (i >= total or edges[i][0] > y or active[li][2] < edges[i][2]):
                cur = active[li]
                li += 1
            else:                                             # insert new edge into active list if y reaches its upper point
                cur = edges[i]
                i += 1
            merged.append(cur)
            if draw:
                if y >= 0:
                    xa, xb = (cur[2], keep[2]) if keep[2] > cur[2] else (keep[2], cur[2])
                    xa, xb = xa >> XY_SHIFT, xb >> XY_SHIFT
                    if xa < w and xb >= 0:
                        img[y, max(xa, 0):min(xb, w - 1) + 1] = color
                keep[2] += keep[3]
                cur[2] += cur[3]
            draw ^= 1
        active = sorted(merged, key=lambda e: e[2])           # the bubble sort of the active list (stable, like it)


def fill_poly(img, pts, color=1):
    """cv2.fillPoly(img, pts, color) for a 2-D uint8 image; pts: iterable of (k, 2) int32 contours (a (1, k, 2) array is one contour)."""
    edges = []
    for c in pts:
        c = np.asarray(c).reshape(-1, 2)
        if len(c):
            edges += _collect_poly_edges(img, c, color)
    _fill_edge_collection(img, edges, color)
    return img


# ---- ultralytics.data.utils ---------------------------------------------------------------------------------------------------------------
def _cv2_resize(src, dsize):
    from oracle import thirdparty as tp

    return tp.cv2_resize(src, dsize, interpolation=1)


def polygon2mask(imgsz, polygons, color=1, downsample_ratio=1, _fill=None, _resize=None):
    mask = np.zeros(imgsz, dtype=np.uint8)
    polygons = np.asarray(polygons, dtype=np.int32)
    polygons = polygons.reshape((polygons.shape[0], -1, 2))
    (_fill or fill_poly)(mask, polygons, color=color)
    nh, nw = (imgsz[0] // downsample_ratio, imgsz[1] // downsample_ratio)
    return (_resize or _cv2_resize)(mask, (nw, nh))


def polygons2masks(imgsz, polygons, color, downsample_ratio=1):
    return np.array([polygon2mask(imgsz, [x.reshape(-1)], color, downsample_ratio) for x in polygons])


def polygons2masks_overlap(imgsz, segments, downsample_ratio=1):
    masks = np.zeros((imgsz[0] // downsample_ratio, imgsz[1] // downsample_ratio), dtype=np.int32 if len(segments) > 255 else np.uint8)
    areas = []
    ms = []
    for si in range(len(segments)):
        mask = polygon2mask(imgsz, [segments[si].reshape(-1)], downsample_ratio=downsample_ratio, color=1)
        ms.append(mask.astype(masks.dtype))
        areas.append(mask.sum())
    areas = np.asarray(areas)
    index = np.argsort(-areas)
    ms = np.array(ms)[index]
    for i in range(len(segments)):
        mask = ms[i] * (i + 1)
        masks = masks + mask
        masks = np.clip(masks, a_min=0, a_max=i + 1)
    return masks, index


def areas_distinct(imgsz, segments, downsample_ratio=1):
    """The condition under which np.argsort(-areas) of polygons2masks_overlap has ONE answer: no two instances of equal shrunk area."""
    a = [int(polygon2mask(imgsz, [s.reshape(-1)], downsample_ratio=downsample_ratio).sum()) for s in segments]
    return len(set(a)) == len(a)


def area_order(areas):
    """The contract of y5_polygon_masks for one image: ascending key -areas in uint64 (zero area wraps to key 0 = first), ties by label index."""
    key = (-np.asarray(areas, dtype=np.uint64)).astype(np.uint64) if len(areas) else np.zeros(0, np.uint64)
    return np.argsort(key, kind="stable")


def reference_masks(xy_list, inst_img, B, H, W, ratio, overlap, flip=None):
    """What y5_polygon_masks computes, from the restatements: xy_list float (k, 2) arrays in label order, inst_img non-decreasing.
    Returns (masks, order, area): masks (n, h, w) uint8 0/1, or (B, h, w) index planes (uint8 up to 255 instances per image, else float32);
    order (n,) per-image permutations (local indices), area (n,)."""
    h, w = H // ratio, W // ratio
    n = len(xy_list)
    flip = np.zeros((B, 2), np.uint8) if flip is None else np.asarray(flip)
    planes = [polygon2mask((H, W), [np.asarray(p).reshape(-1)], downsample_ratio=ratio) for p in xy_list]
    area = np.array([int(p.sum()) for p in planes], np.int64)
    order = np.zeros(n, np.int32)
    inst_img = np.asarray(inst_img, np.int64)

    def flipped(m, b):
        m = m[::-1] if flip[b, 0] else m
        return m[:, ::-1] if flip[b, 1] else m

    if not overlap:
        out = np.zeros((n, h, w), np.uint8)
        for i in range(n):
            out[i] = flipped(planes[i], inst_img[i])
        for b in range(B):
            ids = np.nonzero(inst_img == b)[0]
            order[ids] = area_order(area[ids])
        return out, order, area
    big = any(int((inst_img == b).sum()) > 255 for b in range(B))
    out = np.zeros((B, h, w), np.float32 if big else np.uint8)
    for b in range(B):
        ids = np.nonzero(inst_img == b)[0]
        o = area_order(area[ids])
        order[ids] = o
        m = np.zeros((h, w), np.int64)
        for rank, k in enumerate(o):
            m[planes[ids[k]] != 0] = rank + 1
        out[b] = flipped(m, b)
    return out, order, area


# ---- geometry check that does not rest on the restatement ------------------------------------------------------------------------------
def _cheb_dist_to_segment_le1(px, py, ax, ay, bx, by):
    """True where the Chebyshev distance from integer points (px, py) to the closed segment a-b is <= 1: the square [p - 1, p + 1] meets
    the segment (exact rational clipping in integers: Liang-Barsky with cross-multiplied comparisons)."""
    dx, dy = bx - ax, by - ay
    # parameter interval [t0, t1] = [n0 / d0, n1 / d1] kept as fractions with positive denominators
    ok = np.ones(px.shape, bool)
    n0, d0 = np.zeros(px.shape, np.int64), np.ones(px.shape, np.int64)
    n1, d1 = np.ones(px.shape, np.int64), np.ones(px.shape, np.int64)
    for p, q in ((-dx, ax - (px - 1)), (dx, (px + 1) - ax), (-dy, ay - (py - 1)), (dy, (py + 1) - ay)):
        p = np.broadcast_to(np.int64(p), px.shape)
        q = q.astype(np.int64)
        ok &= ~((p == 0) & (q < 0))
        neg, pos = p < 0, p > 0
        # t >= q / p for p < 0 (numerator -q over -p), t <= q / p for p > 0
        num, den = np.where(neg, -q, q), np.where(neg, -p, np.where(pos, p, 1))
        upd0 = neg & (num * d0 > n0 * den)
        n0, d0 = np.where(upd0, num, n0), np.where(upd0, den, d0)
        upd1 = pos & (num * d1 < n1 * den)
        n1, d1 = np.where(upd1, num, n1), np.where(upd1, den, d1)
    return ok & (n0 * d1 <= n1 * d0)


def check_fill_geometry(mask, pts):
    """mask: (H, W) 0/1 filled from the INTEGER convex polygon pts (k, 2), counter-clockwise or clockwise.  Asserts: every lattice point
    strictly inside (exact cross products) is set; no set pixel lies more than one pixel (Chebyshev) from the closed polygon."""
    H, W = mask.shape
    pts = np.asarray(pts, np.int64)
    k = len(pts)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.int64)
    cr = [(pts[(i + 1) % k, 0] - pts[i, 0]) * (yy - pts[i, 1]) - (pts[(i + 1) % k, 1] - pts[i, 1]) * (xx - pts[i, 0]) for i in range(k)]
    strictly = np.all([c > 0 for c in cr], 0) | np.all([c < 0 for c in cr], 0)
    closed = np.all([c >= 0 for c in cr], 0) | np.all([c <= 0 for c in cr], 0)
    assert mask[strictly].all(), "a lattice point strictly inside the polygon is not set"
    near = closed.copy()
    for i in range(k):
        near |= _cheb_dist_to_segment_le1(xx, yy, *pts[i], *pts[(i + 1) % k])
    assert not (mask.astype(bool) & ~near).any(), "a set pixel lies more than one pixel from the polygon"


def convex_polygons(n, size, seed):
    """n seeded convex integer polygons inside a size x size plane (points on an ellipse, rounded, de-duplicated, convex hull)."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        k = int(rng.integers(3, 9))
        c = rng.uniform(0.3, 0.7, 2) * size
        r = rng.uniform(0.08, 0.3, 2) * size
        a = np.sort(rng.uniform(0, 2 * np.pi, k))
        p = np.unique(np.round(np.stack((c[0] + r[0] * np.cos(a), c[1] + r[1] * np.sin(a)), 1)).astype(np.int64), axis=0)
        hull = _hull(p)
        if len(hull) >= 3:
            out.append(hull)
    return out


def _hull(p):
    p = sorted(map(tuple, p))

    def half(seq):
        o = []
        for q in seq:
            while len(o) >= 2 and (o[-1][0] - o[-2][0]) * (q[1] - o[-2][1]) - (o[-1][1] - o[-2][1]) * (q[0] - o[-2][0]) <= 0:
                o.pop()
            o.append(q)
        return o[:-1]

    return np.array(half(p) + half(p[::-1]), np.int64).reshape(-1, 2)


# ---- data -----------------------------------------------------------------------------------------------------------------------------------
# polygon templates in the unit square of their label box: convex, concave, thin, self-touching (two triangles sharing a vertex)
TEMPLATES = (
    ((0.5, 0.0), (1.0, 0.4), (0.8, 1.0), (0.2, 1.0), (0.0, 0.4)),
    ((0.0, 0.0), (1.0, 0.0), (1.0, 0.3), (0.35, 0.3), (0.35, 1.0), (0.0, 1.0)),
    ((0.0, 0.45), (1.0, 0.5), (0.0, 0.55)),
    ((0.0, 0.0), (0.5, 0.5), (1.0, 0.0), (1.0, 1.0), (0.5, 0.5), (0.0, 1.0)),
    ((0.5, 0.0), (0.62, 0.38), (1.0, 0.38), (0.7, 0.62), (0.8, 1.0), (0.5, 0.77), (0.2, 1.0), (0.3, 0.62), (0.0, 0.38), (0.38, 0.38)),
)


def polygon_dataset(n=6, seed=3, outside=True, tiny=False):
    """(images, classes, segments) on top of oracle.augment_oracle.synthetic_dataset: every label box of that dataset carries one template
    polygon (float32, normalised xy, like the reference's label cache); with `outside`, the polygons of image 1 are pushed partly out of the
    image; with `tiny`, image 2 gets one more polygon of a fraction of a pixel, which vanishes at mask_ratio 4."""
    from oracle import augment_oracle as ao

    ims, labs = ao.synthetic_dataset(n, seed=seed)
    classes, segments = [], []
    for i, lb in enumerate(labs):
        segs, cls = [], []
        for k, (c, xc, yc, w, h) in enumerate(lb):
            t = np.array(TEMPLATES[(i + 2 * k) % len(TEMPLATES)], np.float64)
            # distinct sizes (no two instances of a mosaic may end with equal areas): shrink by a per-(image, label) factor
            f = 1.0 - 0.07 * ((3 * i + 5 * k) % 7)
            p = np.array([xc, yc]) + (t - 0.5) * np.array([w, h]) * f
            if outside and i == 1:
                p = p + np.array([0.35, -0.3]) * (1 if k % 2 == 0 else -1)
            segs.append(p.astype(np.float32))
            cls.append(float(c))
        if tiny and i == 2:
            segs.append((np.array([[0.5, 0.5], [0.503, 0.5], [0.503, 0.504]]) + 0.0017).astype(np.float32))
            cls.append(7.0)
        classes.append(np.array(cls, np.float32))
        segments.append(segs)
    return ims, classes, segments


def ragged_cases(H=64, W=64):
    """Polygons of the direct y5_polygon_masks test: (name, list of (xy float64 (k, 2), image))."""
    sq = lambda x0, y0, x1, y1: np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], np.float64)  # noqa: E731
    rng = np.random.default_rng(11)
    blob = lambda k, c, r: np.stack((c[0] + r * np.cos(np.linspace(0, 2 * np.pi, k, endpoint=False)) * rng.uniform(0.5, 1, k),  # noqa: E731
                                     c[1] + r * np.sin(np.linspace(0, 2 * np.pi, k, endpoint=False)) * rng.uniform(0.5, 1, k)), 1)
    base = [
        (np.array([[10.7, 12.2]]), 0),                                   # single point
        (np.array([[3.0, 40.9], [20.5, 47.1]]), 0),                      # two points
        (sq(-30.0, -30.0, -5.0, -2.0), 0),                               # entirely outside
        (np.array([[-0.9, -0.5], [9.9, -0.2], [4.4, 6.6]]), 0),          # coordinates between -1 and 0 truncate UP to 0
        (sq(30.2, 5.9, 50.8, 25.1), 0),
        (blob(37, (40.0, 44.0), 17.0), 0),                               # ragged, a few tens of points
        (blob(211, (20.0, 30.0), 14.0), 0),                              # a few hundred points, many horizontal micro-edges
        (np.array([[50.0, -20.0], [90.0, 30.0], [40.0, 80.0], [-10.0, 30.0]]), 0),   # partly outside on all four sides
        (np.array([[5.0, 5.0], [30.0, 30.0], [55.0, 5.0], [55.0, 55.0], [30.0, 30.0], [5.0, 55.0]]), 0),  # self-touching
        (sq(20.2, 20.2, 20.9, 20.9), 0),                                 # one pixel: vanishes at ratio 4
        # image 1 has no instance; image 2 has one
        (blob(9, (30.0, 30.0), 25.0), 2),
    ]
    # image 3: more than 255 instances (float32 index planes): a grid of small boxes of DISTINCT areas is impossible at this size, so the
    # tie rule (lower label index first) is exercised here -- against `area_order`, the contract, not against np.argsort
    many = [(sq(2.0 + 3 * (i % 20), 2.0 + 3 * (i // 20), 3.0 + 3 * (i % 20) + (i % 3), 3.0 + 3 * (i // 20) + (i % 2)), 3) for i in range(300)]
    return base + many, 4


def full_size_dataset(n=16, per=8, seed=7, size=(720, 1280)):
    """n frames of `size` with `per` template polygons each (float32 normalised xy, some reaching over the frame border)."""
    from oracle import augment_oracle as ao

    ims, _ = ao.synthetic_dataset(n, seed=seed, sizes=(size,))
    rng = np.random.default_rng(seed)
    classes, segments = [], []
    for i in range(n):
        segs = []
        for k in range(per):
            t = np.array(TEMPLATES[(i + k) % len(TEMPLATES)], np.float64)
            c, wh = rng.uniform(0.1, 0.9, 2), rng.uniform(0.06, 0.4, 2)
            segs.append((c + (t - 0.5) * wh).astype(np.float32))
        classes.append(rng.integers(0, 80, per).astype(np.float32))
        segments.append(segs)
    return ims, classes, segments
