"""Files and shading from the arrays the handles return: a PNG and an OBJ writer and the shading of the surface G-buffer.
numpy only; nothing here touches the library."""
import numpy as np


def write_png(path, rgba, background=(0.0, 0.0, 0.0)):
    """Minimal PNG writer (zlib only): composites straight-alpha RGBA f32 over `background`, 8-bit RGB."""
    import struct
    import zlib
    a = np.clip(rgba[..., 3:4], 0.0, 1.0)
    rgb = np.clip(rgba[..., :3], 0.0, 1.0) * a + np.asarray(background, dtype=np.float32) * (1.0 - a)
    img = (np.clip(rgb, 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)
    h, w = img.shape[:2]
    raw = b"".join(b"\x00" + img[y].tobytes() for y in range(h))

    def chunk(tag, data):
        c = struct.pack(">I", len(data)) + tag + data
        return c + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0))
                + chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


def write_obj(path, vertices, triangles):
    """A mesh of extract_surface as a Wavefront OBJ: one `v` and one `vn` line per vertex, one `f a//a b//b c//c` line per
    triangle, indices 1-based.  Floats are written with nine significant digits (float32 round-trips)."""
    with open(path, "w") as fh:
        for p in vertices["position"]:
            fh.write("v %.9g %.9g %.9g\n" % (p[0], p[1], p[2]))
        for n in vertices["normal"]:
            fh.write("vn %.9g %.9g %.9g\n" % (n[0], n[1], n[2]))
        for t in np.asarray(triangles, dtype=np.int64).reshape(-1, 3) + 1:
            fh.write("f %d//%d %d//%d %d//%d\n" % (t[0], t[0], t[1], t[1], t[2], t[2]))


def surface_hit_points(camera, hits):
    """World positions of a render_surface G-buffer's hits, float32 of the hits' shape + (3,), from the camera and the records' `t`
    (include/fluidsim.h: x(t) = o + t * d; numpy, for shading only).  Pixels without a hit get the ray origin."""
    v3 = lambda a: np.float32([a.x, a.y, a.z])      # noqa: E731
    h, w = hits.shape
    u = ((np.arange(w, dtype=np.float32) + np.float32(0.5)) / np.float32(w) - np.float32(0.5))[None, :, None]
    v = ((np.arange(h, dtype=np.float32) + np.float32(0.5)) / np.float32(h) - np.float32(0.5))[:, None, None]
    span = u * v3(camera.right) + v * v3(camera.up)
    if camera.orthographic:
        o, d = v3(camera.eye) + span, np.broadcast_to(v3(camera.forward), (h, w, 3))
    else:
        o, d = np.broadcast_to(v3(camera.eye), (h, w, 3)), v3(camera.forward) + span
    d = d / np.sqrt((d * d).sum(axis=-1, keepdims=True))
    return (o + hits["t"][..., None] * d).astype(np.float32)


def shade_surface(hits, light=(0.4, -0.8, -0.45), max_speed=None):
    """Lambert shading of a render_surface G-buffer (numpy only): straight-alpha RGBA float32 of the hits' shape, for write_png.
    `light` points from the surface towards the light.  Water blue, tinted towards white by speed (relative to `max_speed`,
    default: the fastest hit); a hit whose first sample was already inside the fluid (hit == 2) is drawn flat and darker."""
    l = np.asarray(light, dtype=np.float32)
    l = l / np.linalg.norm(l)
    lambert = np.clip((hits["normal"] * l).sum(axis=-1), 0.0, 1.0)
    speed = np.sqrt((hits["velocity"].astype(np.float32) ** 2).sum(axis=-1))
    top = float(max_speed) if max_speed else float(speed.max())
    tint = np.clip(speed / top, 0.0, 1.0)[..., None] if top > 0 else np.zeros(hits.shape + (1,), dtype=np.float32)
    base = np.float32([0.10, 0.35, 0.85]) * (1.0 - tint) + np.float32([0.95, 0.97, 1.0]) * tint
    shade = np.where(hits["hit"] == 2, 0.35, 0.25 + 0.75 * lambert)[..., None]
    rgba = np.zeros(hits.shape + (4,), dtype=np.float32)
    rgba[..., 3] = (hits["hit"] != 0).astype(np.float32)
    rgba[..., :3] = base * shade * rgba[..., 3:4]
    return rgba
