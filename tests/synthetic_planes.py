"""Post-pass input planes that a rendered frame never holds (test infrastructure): depths below 16 (what the reference's swapped
pong binding filters on, bilateral_denoise.comp:26 reading the depth image as `center_normal`) clustered in some 32x8 tiles, a
single near pixel in others — at tile corners and on the frame's edges — and none in the rest; depths 16..32767, 32768..65534
(full fog in finalize.comp:44-49) and 0xFFFF; every normal byte; lighting over the whole u16 range with alpha != 4096; albedo,
emission and fog over the whole u8 range, emission non-zero."""
import numpy as np

TILE_W, TILE_H = 32, 8      # the output tile of the LDS-tiled denoise dispatches (rt_post.hip, k_denoise_tiled)


def post_planes(W, H, seed=0):
    """Returns dict(lighting u16[H,W,4], depth u16[H,W], normal u8[H,W], albedo / emission / fog u8[H,W,4])."""
    rng = np.random.default_rng(seed)
    band = rng.integers(0, 4, size=(H, W))
    depth = np.select([band == 0, band == 1, band == 2],
                      [rng.integers(16, 32768, size=(H, W)), rng.integers(32768, 65535, size=(H, W)), rng.integers(16, 2000, size=(H, W))],
                      0xFFFF).astype(np.uint16)
    ty, tx = (H + TILE_H - 1) // TILE_H, (W + TILE_W - 1) // TILE_W
    for j in range(ty):
        for i in range(tx):
            y0, x0 = j * TILE_H, i * TILE_W
            y1, x1 = min(y0 + TILE_H, H), min(x0 + TILE_W, W)
            k = (i + 3 * j) % 4
            if k == 0:            # a cluster of near pixels
                ys, xs = slice(y0, y1), slice(x0 + (x1 - x0) // 3, x0 + 2 * (x1 - x0) // 3 + 1)
                depth[ys, xs] = rng.integers(0, 16, size=depth[ys, xs].shape)
            elif k == 1:          # exactly one near pixel, at one of the tile's corners
                cy, cx = ((y0, x0), (y0, x1 - 1), (y1 - 1, x0), (y1 - 1, x1 - 1))[(i + j) % 4]
                depth[cy, cx] = rng.integers(0, 16)
            # k == 2, 3: no near pixel in the tile
    # single near pixels on the frame's edges (in tiles that have none so far, where the frame is large enough for that)
    for (y, x) in ((0, W // 2), (H - 1, W // 3), (H // 2, 0), (H // 3, W - 1)):
        j, i = y // TILE_H, x // TILE_W
        if (i + 3 * j) % 4 >= 2:
            depth[y, x] = rng.integers(0, 16)
    normal = rng.integers(0, 256, size=(H, W)).astype(np.uint8)
    surf = rng.random((H, W)) < 0.6     # mostly the six face normals and the sky's 16, so the edge-stopping weights vary
    normal[surf] = rng.choice(np.array([0, 1, 2, 3, 4, 5, 16], dtype=np.uint8), size=int(surf.sum()))
    lighting = rng.integers(0, 65536, size=(H, W, 4)).astype(np.uint16)
    lighting[..., 3][lighting[..., 3] == 4096] = 4097
    albedo = rng.integers(0, 256, size=(H, W, 4)).astype(np.uint8)
    emission = rng.integers(0, 256, size=(H, W, 4)).astype(np.uint8)
    emission[..., :3][emission[..., :3].max(axis=-1) == 0] = 1
    fog = rng.integers(0, 256, size=(H, W, 4)).astype(np.uint8)
    return dict(lighting=lighting, depth=depth, normal=normal, albedo=albedo, emission=emission, fog=fog)


def near_pixels_moved_by_the_pong_passes(po, p):
    """In the faithful chain the pong dispatches filter exactly the pixels whose DEPTH is below 16: moving those pixels' depths
    to 16 must change their result (test_post_passes.test_denoise_pong_quirk's method).  Returns the number of near pixels
    whose denoised lighting changed."""
    near = p["depth"] < 16
    far = p["depth"].copy()
    far[near] = 16
    a = po.denoise(p["lighting"], p["depth"], p["normal"], faithful=True)
    b = po.denoise(p["lighting"], far, p["normal"], faithful=True)
    return int((a[near] != b[near]).any(axis=-1).sum())
