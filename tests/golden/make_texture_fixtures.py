"""Generates the image fixtures of the texture tests in this directory: one 4 x 3 image three times over - a binary PPM, an RGB
PNG (colour type 2; scanline filters None, Sub, Up) and an RGBA PNG (colour type 6; filters Average, Paeth, Sub; an alpha that
varies, which a texture ignores).  The same texels in all three: tests/test_gpu_textures_cli.py holds the command line's two
decoders to each other with them.  Standard library only.

Run from the repo root:  python tests/golden/make_texture_fixtures.py"""
import os
import struct
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
W, H = 4, 3


def texel(x, y):
    """(r, g, b, a) of pixel (x, y), row 0 the top row: no two alike, both ends of the byte range present."""
    return ((x * 85) & 255, (y * 127 + 1) & 255, (255 - 40 * x - 13 * y) & 255, (17 + 60 * x + 5 * y) & 255)


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else b if pb <= pc else c


def _filtered(rows, bpp, filters):
    out, prev = bytearray(), bytes(len(rows[0]))
    for row, f in zip(rows, filters):
        out.append(f)
        for i, v in enumerate(row):
            a = row[i - bpp] if i >= bpp else 0
            b, c = prev[i], prev[i - bpp] if i >= bpp else 0
            pred = (0, a, b, (a + b) // 2, _paeth(a, b, c))[f]
            out.append((v - pred) & 255)
        prev = row
    return bytes(out)


def _chunk(tag, body):
    return struct.pack(">I", len(body)) + tag + body + struct.pack(">I", zlib.crc32(tag + body) & 0xFFFFFFFF)


def png(channels, filters):
    rows = [bytes(v for x in range(W) for v in texel(x, y)[:channels]) for y in range(H)]
    idat = zlib.compress(_filtered(rows, channels, filters), 9)
    half = len(idat) // 2                                     # (two IDAT chunks: one zlib stream)
    return (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2 if channels == 3 else 6, 0, 0, 0)) +
            _chunk(b"tEXt", b"Comment\x00texture fixture") + _chunk(b"IDAT", idat[:half]) + _chunk(b"IDAT", idat[half:]) + _chunk(b"IEND", b""))


def main():
    with open(os.path.join(HERE, "checker_4x3.ppm"), "wb") as f:
        f.write(b"P6\n# texture fixture\n%d %d\n255\n" % (W, H) + bytes(v for y in range(H) for x in range(W) for v in texel(x, y)[:3]))
    with open(os.path.join(HERE, "checker_4x3.png"), "wb") as f:
        f.write(png(3, (0, 1, 2)))
    with open(os.path.join(HERE, "checker_4x3_rgba.png"), "wb") as f:
        f.write(png(4, (3, 4, 1)))


if __name__ == "__main__":
    main()
