"""Rules A1-A5 of include/neuman_hip.h 'mesh atlas' in numpy, parametrised by dtype as mesh_lattice_ref is: the float32 run is what
nm_mesh_atlas_pack and nm_mesh_atlas_sample must give bit for bit (a NaN for a NaN), the float64 run is the yardstick of the derived
statements.  `pack` is written in scatter form -- face by face, node by node -- where the device gathers texel by texel, and counts its
writes.  Below the rules: a plain bilinear viewer (`viewer_sample`: texture coordinates -> colour, knowing nothing of blocks or faces) and a
small parser of the three files neuman_hip.mesh_export.write_obj writes."""
import os

import numpy as np

import mesh_lattice_ref as LR

LOWER_NODE, LOWER_GUTTER, UPPER_GUTTER, UPPER_NODE = 0, 1, 2, 3
MAX_SIDE = 16384


# ---- A1 --------------------------------------------------------------------------------------------------------------------------------------
def block(R):
    """-> (BW, BH)"""
    return R + 4, R + 1


def atlas_size(F, R):
    """-> (W, H, nbx), or None where the rule refuses (F < 1, R outside [1, 64], a side above 16384)"""
    if F < 1 or not 1 <= R <= 64:
        return None
    BW, BH = block(R)
    P = (F + 1) // 2
    nbx = 1
    while nbx * nbx * BW < P * BH:                                                      # Python integers: exact at any size
        nbx += 1
        if nbx * BW > MAX_SIDE:
            return None
    nby = -(-P // nbx)
    W, H = nbx * BW, nby * BH
    return None if W > MAX_SIDE or H > MAX_SIDE else (W, H, nbx)


def block_origin(p, R, nbx):
    BW, BH = block(R)
    return (p % nbx) * BW, (p // nbx) * BH


# ---- A2 --------------------------------------------------------------------------------------------------------------------------------------
def classify(R):
    """[BH,BW] int: which of the four sets each texel (x, y) of a block belongs to, by the sum x + y alone"""
    BW, BH = block(R)
    s = np.arange(BW)[None, :] + np.arange(BH)[:, None]
    return np.select([s <= R, s == R + 1, s == R + 2], [LOWER_NODE, LOWER_GUTTER, UPPER_GUTTER], UPPER_NODE)


def place(f, x, y, R, nbx):
    """face f's own local texel (x, y) -> its place (X, Y) in the atlas: the block's origin plus (x, y), reflected for an odd face"""
    f, x, y = np.asarray(f, np.int64), np.asarray(x, np.int64), np.asarray(y, np.int64)
    x0, y0 = block_origin(f // 2, R, nbx)
    odd = f % 2 == 1
    return x0 + np.where(odd, R + 3 - x, x), y0 + np.where(odd, R - y, y)


def owners(F, R):
    """-> (owner [H,W] int: the face whose half block each texel of the atlas lies in, -1 where there is none; kind [H,W]: `classify` of the
    texel inside its block).  Gather form: from the texel to the face."""
    W, H, nbx = atlas_size(F, R)
    BW, BH = block(R)
    Y, X = np.indices((H, W))
    kind = classify(R)[Y % BH, X % BW]
    owner = 2 * ((Y // BH) * nbx + X // BW) + (kind >= UPPER_GUTTER)
    return np.where(owner < F, owner, -1), kind


# ---- A3 --------------------------------------------------------------------------------------------------------------------------------------
def pack(face_colours, R, dtype=np.float32):
    """face_colours [F,S,3] -> (atlas [H,W,3] in `dtype`, writes [H,W] int: how often each texel was assigned; a texel no face owns stays
    +0.0 with 0 writes)"""
    T = np.dtype(dtype).type
    lat = np.asarray(face_colours).astype(T)
    F = lat.shape[0]
    W, H, nbx = atlas_size(F, R)
    atlas, writes = np.zeros((H, W, 3), T), np.zeros((H, W), np.int64)
    faces = np.arange(F)

    def put(x, y, value):
        X, Y = place(faces, x, y, R, nbx)
        atlas[Y, X] = value
        np.add.at(writes, (Y, X), 1)

    c = lambda i1, i2: lat[:, LR.node_index(R, i1, i2)]                                # noqa: E731
    for i2 in range(R + 1):
        for i1 in range(R + 1 - i2):
            put(i1, i2, c(i1, i2))                                                     # a node texel: a copy
    with np.errstate(all='ignore'):
        for x in range(1, R + 1):
            y = R + 1 - x
            put(x, y, (c(x, y - 1) + c(x - 1, y)) - c(x - 1, y - 1))                   # a gutter texel
    put(R + 1, 0, c(R, 0))                                                             # the corner gutter texel
    return atlas, writes


# ---- A4 --------------------------------------------------------------------------------------------------------------------------------------
def uvs(F, R):
    """-> float64 [F,3,2]: (u, v) of the corners (0, 0), (R, 0), (0, R) of every face, texel centres, v up"""
    W, H, nbx = atlas_size(F, R)
    out = np.empty((F, 3, 2))
    for k, (i1, i2) in enumerate(((0, 0), (R, 0), (0, R))):
        X, Y = place(np.arange(F), i1, i2, R, nbx)
        out[:, k, 0] = (X + 0.5) / W
        out[:, k, 1] = 1.0 - (Y + 0.5) / H
    return out


# ---- A5 --------------------------------------------------------------------------------------------------------------------------------------
def sample(atlas, F, R, face_id, b1, b2, dtype=np.float32):
    """-> (colour [n,3] in `dtype`, info: dict of i1, i2 [n] int, f1, f2 [n], D [n,3] = t00 - t10 - t01 + t11 in `dtype`, valid [n] bool,
    X, Y [n,4]: the texels read (t00, t10, t01, t11; 0 where not valid))"""
    T = np.dtype(dtype).type
    img = np.asarray(atlas)
    W, H, nbx = atlas_size(F, R)
    assert img.shape == (H, W, 3)
    face_id = np.asarray(face_id, np.int64)
    valid = (face_id >= 0) & (face_id < F)
    f = np.where(valid, face_id, 0)
    with np.errstate(all='ignore'):
        u1, u2 = np.asarray(b1).astype(T) * T(R), np.asarray(b2).astype(T) * T(R)
        i1 = np.clip(np.where(np.isnan(u1), 0, np.floor(u1)), 0, R - 1).astype(np.int64)
        i2 = np.clip(np.where(np.isnan(u2), 0, np.floor(u2)), 0, R - 1 - i1).astype(np.int64)
        f1, f2 = u1 - i1.astype(T), u2 - i2.astype(T)
        g1, g2 = T(1) - f1, T(1) - f2
        w = [(g1 * g2)[:, None], (f1 * g2)[:, None], (g1 * f2)[:, None], (f1 * f2)[:, None]]
        at = [place(f, i1 + a, i2 + b, R, nbx) for a, b in ((0, 0), (1, 0), (0, 1), (1, 1))]
        t = [img[Y, X].astype(T) for X, Y in at]
        colour = (w[0] * t[0] + w[1] * t[1]) + (w[2] * t[2] + w[3] * t[3])
        D = ((t[0] - t[1]) - t[2]) + t[3]
    colour = np.where(valid[:, None], colour, T(0)).astype(T)
    X, Y = (np.where(valid[:, None], np.stack([a[k] for a in at], 1), 0) for k in (0, 1))
    return colour, dict(i1=i1, i2=i2, f1=f1, f2=f2, D=D.astype(T), valid=valid, X=X, Y=Y)


def same_values(a, b):
    """same shape, a NaN exactly where the other has one, and the same bits everywhere else (a NaN's payload and sign are not the rules')"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint8), b[~nb].view(np.uint8)))


# ---- a viewer ----------------------------------------------------------------------------------------------------------------------------------
def viewer_sample(image, uv):
    """Bilinear filtering as an OBJ viewer does it, in float64: image [H,W,C] (row 0 on top), uv [n,2] with v up; texel centres at half
    integers, coordinates clamped to the image's edge -> [n,C]"""
    img = np.asarray(image).astype(np.float64)
    H, W = img.shape[:2]
    uv = np.asarray(uv, np.float64)
    x = np.clip(uv[:, 0] * W - 0.5, 0, W - 1)
    y = np.clip((1.0 - uv[:, 1]) * H - 0.5, 0, H - 1)
    x0, y0 = np.minimum(np.floor(x).astype(np.int64), max(W - 2, 0)), np.minimum(np.floor(y).astype(np.int64), max(H - 2, 0))
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    fx, fy = (x - x0)[:, None], (y - y0)[:, None]
    return (img[y0, x0] * (1 - fx) + img[y0, x1] * fx) * (1 - fy) + (img[y1, x0] * (1 - fx) + img[y1, x1] * fx) * fy


# ---- the three files ---------------------------------------------------------------------------------------------------------------------------
def read_obj(path):
    """-> dict(mtllib, usemtl: str; v [V,3], vn [N,3], vt [T,2] float64; f_v, f_t [F,3] int64 0-based, f_n [F,3] or None)"""
    out = dict(mtllib=None, usemtl=None, v=[], vn=[], vt=[], f=[])
    with open(path) as src:
        for line in src:
            word = line.split()
            if not word or word[0].startswith('#'):
                continue
            if word[0] in ('mtllib', 'usemtl'):
                out[word[0]] = word[1]
            elif word[0] in ('v', 'vn', 'vt'):
                out[word[0]].append([float(x) for x in word[1:]])
            elif word[0] == 'f':
                out['f'].append([[int(i) - 1 for i in corner.split('/')] for corner in word[1:]])
            else:
                raise ValueError(f"{path}: a line of kind {word[0]!r}")
    f = np.array(out.pop('f'), np.int64)                                               # [F,3,2 or 3]
    out.update(v=np.array(out['v']).reshape(-1, 3), vn=np.array(out['vn']).reshape(-1, 3), vt=np.array(out['vt']).reshape(-1, 2), f_v=f[..., 0],
               f_t=f[..., 1], f_n=f[..., 2] if f.shape[-1] == 3 else None)
    return out


def read_mtl(path):
    """-> {material: {key: the rest of the line}}"""
    out, cur = {}, None
    with open(path) as src:
        for line in src:
            word = line.split(None, 1)
            if not word or word[0].startswith('#'):
                continue
            if word[0] == 'newmtl':
                cur = out.setdefault(word[1].strip(), {})
            else:
                cur[word[0]] = word[1].strip()
    return out


def read_png(path):
    """-> uint8 [H,W,3] (Pillow's decoder)"""
    from PIL import Image
    with Image.open(path) as im:
        return np.array(im.convert('RGB'))


def read_export(obj_path):
    """the .obj, the .mtl it names and the image that names -> (obj dict, image uint8 [H,W,3])"""
    obj = read_obj(obj_path)
    here = os.path.dirname(obj_path)
    mtl = read_mtl(os.path.join(here, obj['mtllib']))
    return obj, read_png(os.path.join(here, mtl[obj['usemtl']]['map_Kd']))
