"""NumPy restatement of sequence inference with symmetry averaging
(unet_amd.predict, csrc/predict.hip): the symmetry maps and their inverses,
the work list, the gather (on unet_amd.tiling.mirror_index) and the reduce in
float64.  Written from the definition (np.rot90 / np.flip), not from the
kernels' index algebra."""
import numpy as np

from types import SimpleNamespace

from unet_amd.tiling import mirror_index, output_size

SETS = {"none": (0,), "flip": (0, 4), "rot4": (0, 1, 2, 3), "d4": tuple(range(8))}


def sym(x, s):
    """S_s(x) = rot90(flip_f(x), r), s = r + 4 f, on the last two axes."""
    r, f = s & 3, s >> 2
    return np.rot90(np.flip(x, -1) if f else x, r, (-2, -1))


def sym_inv(y, s):
    r, f = s & 3, s >> 2
    x = np.rot90(y, -r, (-2, -1))
    return np.flip(x, -1) if f else x


def geometry(H, W, tile_in, tile_out=None):
    """The tile grid of an H x W frame: tile_out defaults to the network's; the
    margin (tile_in - tile_out) // 2 is mirrored on the top / left."""
    to = output_size(tile_in) if tile_out is None else tile_out
    ny, nx = -(-H // to), -(-W // to)
    m = (tile_in - to) // 2
    return SimpleNamespace(tile_in=tile_in, tile_out=to, ny=ny, nx=nx, top=m, left=m,
                           origins=[(ty * to, tx * to) for ty in range(ny) for tx in range(nx)])


def work_list(n_frames, n_tiles):
    """frame-major (frame, tile) pairs, (n_frames * n_tiles, 2) int32"""
    return np.array([(f, t) for f in range(n_frames) for t in range(n_tiles)], np.int32).reshape(-1, 2)


def normalise(frames):
    """predict.py's ToTensor + Normalize(0.5, 0.5) in fp32; fp32 is passed on"""
    if frames.dtype == np.uint8:
        x = frames.astype(np.float32) / np.float32(255)
        return ((x - np.float32(0.5)) / np.float32(0.5)).astype(np.float32)
    return frames


def gather(frames, tile_in, work, codes, tile_out=None):
    """frames (F, C, H, W) -> tiles (G * ns, C, ti, ti): entry g * ns + j is
    S_{codes[j]} of the mirror-folded tile of group g."""
    F, C, H, W = frames.shape
    geo = geometry(H, W, tile_in, tile_out)
    x = normalise(frames)
    out = np.empty((len(work) * len(codes), C, tile_in, tile_in), np.float32)
    for g, (f, t) in enumerate(work):
        oy, ox = geo.origins[t]
        iy = mirror_index(tile_in, oy - geo.top, H).numpy()
        ix = mirror_index(tile_in, ox - geo.left, W).numpy()
        tile = x[f][:, iy][:, :, ix]
        for j, s in enumerate(codes):
            out[g * len(codes) + j] = sym(tile, s)
    return out


def mean_softmax_tiles(logits, ns, codes):
    """logits (G * ns, K, to, to) -> (G, K, to, to) float64: the mean over j of
    S^-1 of the softmax of entry g * ns + j"""
    lt = logits.astype(np.float64)
    e = np.exp(lt - lt.max(1, keepdims=True))
    p = e / e.sum(1, keepdims=True)
    G = len(lt) // ns
    return np.stack([sum(sym_inv(p[g * ns + j], s) for j, s in enumerate(codes)) / ns for g in range(G)])


def reduce(logits, work, codes, F, H, W, tile_in, tile_out=None, fill=np.nan):
    """The mean probabilities (F, K, H, W) float64; pixels of no listed tile
    hold `fill`."""
    geo = geometry(H, W, tile_in, tile_out)
    to = geo.tile_out
    K = logits.shape[1]
    pm = mean_softmax_tiles(logits, len(codes), codes)
    full = np.full((F, K, geo.ny * to, geo.nx * to), fill, np.float64)
    for g, (f, t) in enumerate(work):
        y, x = geo.origins[t]
        full[f, :, y:y + to, x:x + to] = pm[g]
    return full[:, :, :H, :W]
