"""Cuts the top rows out of the reference's committed render (rtiow_part1_final.png, 1200x800 RGBA8, 1.3 MB: too
large to commit) into tests/golden/ref_png_head.png, the input of test_host_scene.py's read_png test.

The scanlines are kept exactly as the reference's encoder (the `image` crate) filtered them, filter-type bytes included;
only the DEFLATE stream is redone (zlib, level 9) and IHDR's height cut to the rows kept.  A PNG scanline is filtered
against the one above it, so the cut keeps rows 0..K-1: every row of ref_png_sky_rows.json, and at least one scanline
of each filter type the encoder used anywhere in the image.

Run once, with the reference's PNG at hand:
    python tests/golden/make_ref_png_head.py path/to/rtiow_part1_final.png
"""
import json
import os
import struct
import sys
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
DST = os.path.join(HERE, "ref_png_head.png")


def chunks(data):
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos = 8
    while pos < len(data):
        n, = struct.unpack(">I", data[pos:pos + 4])
        yield data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        pos += 12 + n


def main(src):
    cs = list(chunks(open(src, "rb").read()))
    ihdr = dict(cs)[b"IHDR"]
    w, h, depth, ctype, comp, filt, interlace = struct.unpack(">IIBBBBB", ihdr)
    assert (w, h, depth, ctype, interlace) == (1200, 800, 8, 6, 0), (w, h, depth, ctype, interlace)
    stride = 1 + w * 4
    raw = zlib.decompress(b"".join(d for t, d in cs if t == b"IDAT"))
    assert len(raw) == h * stride
    types = [raw[y * stride] for y in range(h)]
    fx = json.load(open(os.path.join(HERE, "ref_png_sky_rows.json")))
    last_row = max([int(y) for y in fx["constant_rows"]] + [p["y"] for p in fx["points"]])
    k = max([last_row] + [types.index(t) for t in set(types)]) + 1
    chunk = lambda t, d: struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d) & 0xFFFFFFFF)
    out = (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, k, depth, ctype, comp, filt, interlace))
           + chunk(b"IDAT", zlib.compress(raw[:k * stride], 9)) + chunk(b"IEND", b""))
    open(DST, "wb").write(out)
    print(f"wrote {DST}: rows 0..{k - 1} of {h}, filter types {sorted(set(types[:k]))}, {len(out)} bytes")


if __name__ == "__main__":
    main(sys.argv[1])
