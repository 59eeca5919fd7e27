"""A PNG writer and reader for the two formats the stored results need - 8-bit RGB and 16-bit RGB - on zlib and struct alone.
PIL cannot write 16-bit RGB, and the reference's cv2 / imageio are not dependencies of this package.  The reader reads what the
writer writes (colour type 2, no interlace, any of the five row filters) and is meant for tests and for checking a submission."""
import struct
import zlib

import numpy as np

_SIG = b"\x89PNG\r\n\x1a\n"


def _chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def encode_png(img, level=6):
    """The bytes of a PNG file of `img`: (H, W, 3) uint8 or uint16 (stored big-endian, as the format asks).  Filter 0 on every row."""
    img = np.asarray(img)
    if img.ndim != 3 or img.shape[2] != 3 or img.dtype not in (np.uint8, np.uint16) or img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError(f"encode_png: an (H, W, 3) uint8 or uint16 array, got {img.shape} {img.dtype}")
    H, W, _ = img.shape
    depth = 8 * img.dtype.itemsize
    rows = np.ascontiguousarray(img.astype(">u2") if depth == 16 else img).view(np.uint8).reshape(H, -1)
    raw = np.concatenate((np.zeros((H, 1), np.uint8), rows), axis=1).tobytes()
    ihdr = struct.pack(">IIBBBBB", W, H, depth, 2, 0, 0, 0)
    return _SIG + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", zlib.compress(raw, level)) + _chunk(b"IEND", b"")


def write_png(path, img, level=6):
    with open(path, "wb") as f:
        f.write(encode_png(img, level))


def _unfilter(raw, H, stride, bpp):
    out = np.zeros((H, stride), np.uint8)
    prev = np.zeros(stride, np.int64)
    for y in range(H):
        f = raw[y * (stride + 1)]
        line = np.frombuffer(raw, np.uint8, stride, y * (stride + 1) + 1).astype(np.int64)
        if f == 0:
            cur = line
        elif f == 2:
            cur = (line + prev) & 255
        else:
            cur = np.zeros(stride, np.int64)
            for i in range(stride):
                a = cur[i - bpp] if i >= bpp else 0
                b = prev[i]
                c = prev[i - bpp] if i >= bpp else 0
                if f == 1:
                    p = a
                elif f == 3:
                    p = (a + b) >> 1
                elif f == 4:
                    pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
                    p = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
                else:
                    raise ValueError(f"read_png: unknown row filter {f}")
                cur[i] = (line[i] + p) & 255
        out[y] = cur
        prev = cur
    return out


def decode_png(data):
    """(H, W, 3) uint8 or uint16 (native byte order) of the bytes of an 8- or 16-bit RGB PNG; every chunk's CRC is checked."""
    if data[:8] != _SIG:
        raise ValueError("read_png: not a PNG file")
    at, idat, head = 8, [], None
    while at < len(data):
        n, tag = struct.unpack(">I4s", data[at:at + 8])
        body = data[at + 8:at + 8 + n]
        if struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] != (zlib.crc32(tag + body) & 0xFFFFFFFF):
            raise ValueError(f"read_png: bad CRC in chunk {tag!r}")
        if tag == b"IHDR":
            head = struct.unpack(">IIBBBBB", body)
        elif tag == b"IDAT":
            idat.append(body)
        elif tag == b"IEND":
            break
        at += 12 + n
    if head is None:
        raise ValueError("read_png: no IHDR chunk")
    W, H, depth, colour, _, _, interlace = head
    if colour != 2 or depth not in (8, 16) or interlace:
        raise ValueError(f"read_png: 8- or 16-bit RGB without interlace only (depth {depth}, colour type {colour}, interlace {interlace})")
    bpp = 3 * depth // 8
    rows = _unfilter(zlib.decompress(b"".join(idat)), H, W * bpp, bpp)
    if depth == 8:
        return rows.reshape(H, W, 3)
    return rows.view(">u2").reshape(H, W, 3).astype(np.uint16)


def read_png(path):
    with open(path, "rb") as f:
        return decode_png(f.read())
