"""evh_jpeg_encode restated in numpy (include/evhip.h, "pictures encoded on the device"): pictures -> file bytes, for EQUALITY
with the library, and a plain baseline decoder written from T.81 that returns the pixels and the quantised coefficients it
read.  Nothing here knows the library; the decoder shares only the Annex K tables and the zig-zag order with the encoder."""
import math
import struct

import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62,
                   63])
# T.81 Annex K.1, K.2 in natural order
K1 = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
               18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112,
               100, 103, 99])
K2 = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] +
              [99] * 32)
# T.81 Annex K.3: (code lengths 1..16, symbols); [0] luminance, [1] chrominance
DC_BITS = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0])
DC_VALS = (list(range(12)), list(range(12)))
AC_BITS = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125], [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119])
AC_VALS = (
    [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
     0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
     0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
     0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
     0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
     0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
     0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa],
    [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
     0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
     0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
     0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
     0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
     0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa])
BLOCK_BITS = 20 + 63 * 26
SUBSAMPLINGS = {"444": 0, "420": 1}


def quant_tables(quality):
    """Annex K.1 / K.2 scaled by the usual rule -> uint16 [2, 64], natural order."""
    q = int(quality)
    s = 5000 // q if q < 50 else 200 - 2 * q
    return np.stack([np.clip((b * s + 50) // 100, 1, 255) for b in (K1, K2)]).astype(np.uint16)


def huffman_codes(bits, vals):
    """Annex C: symbol -> (code, length)."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


DC_CODES = [huffman_codes(DC_BITS[t], DC_VALS[t]) for t in range(2)]
AC_CODES = [huffman_codes(AC_BITS[t], AC_VALS[t]) for t in range(2)]


def _code_arrays(codes, n):
    c, l = np.zeros(n, np.uint64), np.zeros(n, np.int64)
    for sym, (code, length) in codes.items():
        c[sym], l[sym] = code, length
    return c, l


_DC = [_code_arrays(DC_CODES[t], 12) for t in range(2)]
_AC = [_code_arrays(AC_CODES[t], 256) for t in range(2)]

DCT_TABLE = np.array([[int(np.rint(8192 * (1 / math.sqrt(2) if u == 0 else 1.0) / 2 * math.cos((2 * x + 1) * u * math.pi / 16)))
                       for x in range(8)] for u in range(8)], dtype=np.int64)
DCT_FLOAT = np.array([[(1 / math.sqrt(2) if u == 0 else 1.0) / 2 * math.cos((2 * x + 1) * u * math.pi / 16) for x in range(8)]
                      for u in range(8)])


def fdct_int(s):
    """[..., 8, 8] level-shifted samples (y, x) -> F[..., v, u], the two passes of include/evhip.h."""
    s = np.asarray(s, np.int64)
    a = (np.einsum("ux,...yx->...yu", DCT_TABLE, s) + 128) >> 8
    return (np.einsum("vy,...yu->...vu", DCT_TABLE, a) + (1 << 17)) >> 18


def fdct_float(s):
    """The float64 orthonormal DCT-II of the same samples, unrounded."""
    return np.einsum("vy,...yu->...vu", DCT_FLOAT, np.einsum("ux,...yx->...yu", DCT_FLOAT, np.asarray(s, np.float64)))


def fdct_ideal(s):
    """fdct_float rounded to integers: the ideal-arithmetic variant of the quality comparison."""
    return np.rint(fdct_float(s)).astype(np.int64)


def ycc(bgr):
    b, g, r = (bgr[..., c].astype(np.int64) for c in range(3))
    return np.stack([(19595 * r + 38470 * g + 7471 * b + 32768) >> 16,
                     (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16,
                     (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16], axis=-1)


def geometry(w, h, cn, sub):
    """-> (mcu side, blocks per MCU, MCUs per row, MCU rows)"""
    mcu = 16 if sub == 1 else 8
    return mcu, (1 if cn == 1 else 6 if sub == 1 else 3), -(-w // mcu), -(-h // mcu)


def _blocks8(plane, rows, cols):
    """[rows * 8, cols * 8] -> [rows, cols, 8, 8]"""
    return plane.reshape(rows, 8, cols, 8).transpose(0, 2, 1, 3)


def sample_blocks(picture, sub):
    """The level-shifted samples of every block in scan order: [MCU rows, MCUs per row, blocks per MCU, 8, 8]."""
    picture = np.asarray(picture)
    h, w = picture.shape[:2]
    cn = 1 if picture.ndim == 2 else 3
    mcu, bpm, mx, my = geometry(w, h, cn, sub)
    ys, xs = np.minimum(np.arange(my * mcu), h - 1), np.minimum(np.arange(mx * mcu), w - 1)
    padded = picture[ys][:, xs]
    if cn == 1:
        return _blocks8(padded.astype(np.int64) - 128, my, mx)[:, :, None]
    c = ycc(padded) - 128
    if sub == 0:
        return np.stack([_blocks8(c[..., k], my, mx) for k in range(3)], axis=2)
    y = _blocks8(c[..., 0], 2 * my, 2 * mx).reshape(my, 2, mx, 2, 8, 8).transpose(0, 2, 1, 3, 4, 5).reshape(my, mx, 4, 8, 8)
    ch = c[..., 1:] + 128
    ch = ((ch[0::2, 0::2] + ch[0::2, 1::2] + ch[1::2, 0::2] + ch[1::2, 1::2] + 2) >> 2) - 128
    return np.concatenate([y, _blocks8(ch[..., 0], my, mx)[:, :, None], _blocks8(ch[..., 1], my, mx)[:, :, None]], axis=2)


def components(bpm):
    return [0] if bpm == 1 else [0, 1, 2] if bpm == 3 else [0, 0, 0, 0, 1, 2]


def quantise(F, qtabs, bpm):
    """F [rows, mx, bpm, 8, 8] -> quantised coefficients in zig-zag order [rows, mx, bpm, 64]"""
    qt = np.asarray(qtabs, np.int64).reshape(2, 64)
    Q = np.stack([qt[1 if c else 0] for c in components(bpm)]).reshape(bpm, 8, 8)
    mag = (np.abs(F) + (Q >> 1)) // Q
    return (np.sign(F) * mag).reshape(F.shape[:3] + (64,))[..., ZIGZAG]


def _bit_length(a):
    a = np.abs(np.asarray(a, np.int64))
    out = np.zeros(a.shape, np.int64)
    for k in range(12):
        out += (a >> k) > 0
    return out


def header(w, h, cn, sub, qtabs):
    qt = np.asarray(qtabs).reshape(2, 64)
    o = bytearray(b"\xff\xd8\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for t in range(1 if cn == 1 else 2):
        o += bytes([0xFF, 0xDB, 0, 67, t]) + bytes(int(v) for v in qt[t][ZIGZAG])
    o += bytes([0xFF, 0xC0, 0, 8 + 3 * cn, 8, h >> 8, h & 255, w >> 8, w & 255, cn])
    for c in range(cn):
        o += bytes([c + 1, 0x22 if (c == 0 and sub == 1) else 0x11, 1 if c else 0])
    for t in range(2):
        o += bytes([0xFF, 0xC4, 0, 31, t]) + bytes(DC_BITS[t]) + bytes(DC_VALS[t])
        o += bytes([0xFF, 0xC4, 0, 181, 0x10 | t]) + bytes(AC_BITS[t]) + bytes(AC_VALS[t])
    dri = -(-w // (16 if sub == 1 else 8))
    o += bytes([0xFF, 0xDD, 0, 4, dri >> 8, dri & 255])
    o += bytes([0xFF, 0xDA, 0, 6 + 2 * cn, cn])
    for c in range(cn):
        o += bytes([c + 1, 0x11 if c else 0x00])
    return bytes(o + b"\x00\x3f\x00")


def scan_rows(zz):
    """Quantised coefficients [rows, mx, bpm, 64] -> per MCU row its interval's bytes before stuffing (padded with 1-bits).
    Every code of a block is one symbol of up to 59 bits (the ZRLs of a run go with their coefficient's code)."""
    rows, mx, bpm, _ = zz.shape
    comp = np.array(components(bpm))
    tab = (comp > 0).astype(np.int64)
    bpr = mx * bpm
    z = zz.reshape(rows, bpr, 64).astype(np.int64)
    btab = np.tile(tab, mx)                                  # table of each block of a row
    # DC: the difference to the previous block of the same component inside the row
    dc = z[:, :, 0]
    diff = np.zeros_like(dc)
    for c in range(3):
        sel = np.flatnonzero(np.tile(comp, mx) == c)
        if sel.size:
            diff[:, sel] = np.diff(dc[:, sel], axis=1, prepend=0)
    cat = _bit_length(diff)
    tb = np.broadcast_to(btab, cat.shape)
    dcc, dcl = np.stack([_DC[0][0], _DC[1][0]])[tb, cat], np.stack([_DC[0][1], _DC[1][1]])[tb, cat]
    val = np.where(diff < 0, diff - 1, diff) & ((1 << cat) - 1)
    ev_key = [(np.arange(rows)[:, None] * bpr + np.arange(bpr)[None, :]).reshape(-1) * 66]
    ev_code = [((dcc << cat.astype(np.uint64)) | val.astype(np.uint64)).reshape(-1)]
    ev_len = [(dcl + cat).reshape(-1)]
    # AC
    flat = z.reshape(rows * bpr, 64)
    b, k = np.nonzero(flat[:, 1:])
    k = k + 1
    same = np.concatenate([[False], b[1:] == b[:-1]])
    prev = np.where(same, np.concatenate([[0], k[:-1]]), 0)
    run = k - 1 - prev
    v = flat[b, k]
    size = _bit_length(v)
    t = np.tile(btab, rows)[b]
    acc = np.stack([_AC[0][0], _AC[1][0]])
    acl = np.stack([_AC[0][1], _AC[1][1]])
    code = np.zeros(b.size, np.uint64)
    length = np.zeros(b.size, np.int64)
    for zi in range(3):
        more = (run >> 4) > zi
        zl = acl[t, 0xF0]
        code = np.where(more, (code << zl.astype(np.uint64)) | acc[t, 0xF0], code)
        length = length + np.where(more, zl, 0)
    sym = ((run & 15) << 4) | size
    assert np.all(acl[t, sym] > 0)
    code = (code << acl[t, sym].astype(np.uint64)) | acc[t, sym]
    code = (code << size.astype(np.uint64)) | (np.where(v < 0, v - 1, v) & ((1 << size) - 1)).astype(np.uint64)
    length = length + acl[t, sym] + size
    ev_key.append(b * 66 + k)
    ev_code.append(code)
    ev_len.append(length)
    # EOB unless coefficient 63 is non-zero
    eb = np.flatnonzero(flat[:, 63] == 0)
    et = np.tile(btab, rows)[eb]
    ev_key.append(eb * 66 + 64)
    ev_code.append(acc[et, 0])
    ev_len.append(acl[et, 0])
    key, code, length = np.concatenate(ev_key), np.concatenate(ev_code), np.concatenate(ev_len)
    order = np.argsort(key, kind="stable")
    key, code, length = key[order], code[order], length[order]
    row_of = key // (66 * bpr)
    out = []
    for r in range(rows):
        sel = row_of == r
        c, l = code[sel], length[sel]
        total = int(l.sum())
        pad = (-total) % 8
        start = np.cumsum(l) - l
        idx = np.repeat(np.arange(l.size), l)
        j = np.arange(total) - np.repeat(start, l)
        bits = ((c[idx] >> (l[idx] - 1 - j).astype(np.uint64)) & np.uint64(1)).astype(np.uint8)
        bits = np.concatenate([bits, np.ones(pad, np.uint8)])
        out.append(np.packbits(bits).tobytes())
    return out


def assemble(head, rows):
    o = bytearray(head)
    for r, data in enumerate(rows):
        o += data.replace(b"\xff", b"\xff\x00")
        if r < len(rows) - 1:
            o += bytes([0xFF, 0xD0 + (r & 7)])
    return bytes(o + b"\xff\xd9")


def coefficients(picture, qtabs, subsampling="420", dct=fdct_int):
    sub = SUBSAMPLINGS[subsampling] if isinstance(subsampling, str) else int(subsampling)
    s = sample_blocks(picture, sub)
    return quantise(dct(s), qtabs, s.shape[2])


def encode_coefficients(zz, w, h, cn, sub, qtabs):
    return assemble(header(w, h, cn, sub, qtabs), scan_rows(np.asarray(zz)))


def encode(picture, qtabs, subsampling="420", dct=fdct_int):
    """One picture [h, w] gray or [h, w, 3] BGR -> the bytes of its file."""
    picture = np.asarray(picture)
    sub = SUBSAMPLINGS[subsampling] if isinstance(subsampling, str) else int(subsampling)
    h, w = picture.shape[:2]
    return encode_coefficients(coefficients(picture, qtabs, sub, dct), w, h, 1 if picture.ndim == 2 else 3, sub, qtabs)


def bound(w, h, cn, sub):
    mcu, bpm, mx, my = geometry(w, h, cn, sub)
    return (550 if cn == 1 else 629) + my * (2 * ((mx * bpm * BLOCK_BITS + 7) // 8) + 2) + 2


# ---- the decoder: T.81 baseline, nothing shared with the encoder but the tables' source ----------------------------------------
class _Bits:
    def __init__(self, data):
        self.d, self.pos, self.acc, self.n = data, 0, 0, 0

    def bit(self):
        if self.n == 0:
            assert self.pos < len(self.d), "the scan ended inside a code"
            self.acc, self.n = self.d[self.pos], 8
            self.pos += 1
        self.n -= 1
        return (self.acc >> self.n) & 1

    def receive(self, n):
        v = 0
        for _ in range(n):
            v = v << 1 | self.bit()
        return v

    def symbol(self, table):
        code = 0
        for length in range(1, 17):
            code = code << 1 | self.bit()
            if (code, length) in table:
                return table[(code, length)]
        raise AssertionError("no such Huffman code")


def _extend(v, n):
    return v if n == 0 or v >= (1 << (n - 1)) else v - (1 << n) + 1


def parse(data):
    """The segments of a file: {'dqt': {id: natural-order table}, 'dht': {(class, id): {(code, length): symbol}}, 'sof': ...,
    'dri': n, 'sos': [...], 'intervals': [unstuffed bytes], 'rst': [m, ...], 'markers': [...]} -- asserts what baseline needs."""
    data = bytes(data)
    assert data[:2] == b"\xff\xd8", "no SOI"
    out = {"dqt": {}, "dht": {}, "markers": [0xD8], "dri": 0, "dht_raw": {}}
    i = 2
    while True:
        assert data[i] == 0xFF, "marker expected at %d" % i
        m = data[i + 1]
        n = data[i + 2] << 8 | data[i + 3]
        seg = data[i + 4:i + 2 + n]
        out["markers"].append(m)
        if m == 0xE0:
            assert seg[:5] == b"JFIF\x00"
        elif m == 0xDB:
            j = 0
            while j < len(seg):
                assert seg[j] >> 4 == 0, "8-bit tables only"
                t = np.zeros(64, np.int64)
                t[ZIGZAG] = list(seg[j + 1:j + 65])
                out["dqt"][seg[j] & 15] = t
                j += 65
        elif m == 0xC0:
            assert seg[0] == 8
            out["sof"] = {"h": seg[1] << 8 | seg[2], "w": seg[3] << 8 | seg[4],
                          "comps": [(seg[6 + 3 * c], seg[7 + 3 * c] >> 4, seg[7 + 3 * c] & 15, seg[8 + 3 * c]) for c in range(seg[5])]}
        elif m == 0xC4:
            j = 0
            while j < len(seg):
                bits = list(seg[j + 1:j + 17])
                vals = list(seg[j + 17:j + 17 + sum(bits)])
                out["dht"][(seg[j] >> 4, seg[j] & 15)] = {v: k for k, v in huffman_codes(bits, vals).items()}
                out["dht_raw"][(seg[j] >> 4, seg[j] & 15)] = (bits, vals)
                j += 17 + sum(bits)
        elif m == 0xDD:
            out["dri"] = seg[0] << 8 | seg[1]
        elif m == 0xDA:
            out["sos"] = [(seg[1 + 2 * c], seg[2 + 2 * c] >> 4, seg[2 + 2 * c] & 15) for c in range(seg[0])]
            assert tuple(seg[1 + 2 * seg[0]:]) == (0, 63, 0)
            i += 2 + n
            break
        else:
            raise AssertionError("unexpected marker %02x" % m)
        i += 2 + n
    intervals, rst, cur = [], [], bytearray()
    while True:
        assert i < len(data), "no EOI"
        if data[i] != 0xFF:
            cur.append(data[i]); i += 1
        elif data[i + 1] == 0:
            cur.append(0xFF); i += 2
        elif 0xD0 <= data[i + 1] <= 0xD7:
            intervals.append(bytes(cur)); cur = bytearray(); rst.append(data[i + 1] - 0xD0); i += 2
        else:
            assert data[i + 1] == 0xD9 and i + 2 == len(data), "EOI must end the file"
            intervals.append(bytes(cur))
            break
    out["intervals"], out["rst"] = intervals, rst
    return out


def decode(data):
    """-> (pixels uint8 [h, w] or [h, w, 3] BGR, coefficients [MCU rows, MCUs per row, blocks per MCU, 64] zig-zag order, info).
    Dequantise, float64 IDCT rounded and clamped to 8 bits, chroma up-sampling by replication, inverse JFIF colour in float64."""
    P = parse(data)
    w, h, comps = P["sof"]["w"], P["sof"]["h"], P["sof"]["comps"]
    cn = len(comps)
    hmax = max(c[1] for c in comps)
    sub = 1 if hmax == 2 else 0
    assert [c[1:3] for c in comps] == ([(hmax, hmax)] + [(1, 1)] * (cn - 1))
    mcu, bpm, mx, my = geometry(w, h, cn, sub)
    assert P["dri"] == mx and len(P["intervals"]) == my and P["rst"] == [r & 7 for r in range(my - 1)]
    comp_of = components(bpm)
    zz = np.zeros((my, mx, bpm, 64), np.int64)
    pad_bits = []
    for r, data_r in enumerate(P["intervals"]):
        B = _Bits(data_r)
        pred = [0, 0, 0]
        for m in range(mx):
            for k in range(bpm):
                c = comp_of[k]
                td, ta = P["sos"][c][1], P["sos"][c][2]
                n = B.symbol(P["dht"][(0, td)])
                pred[c] += _extend(B.receive(n), n)
                zz[r, m, k, 0] = pred[c]
                pos = 1
                while pos < 64:
                    rs = B.symbol(P["dht"][(1, ta)])
                    if rs == 0:
                        break
                    if rs == 0xF0:
                        pos += 16
                        continue
                    pos += rs >> 4
                    assert pos < 64
                    zz[r, m, k, pos] = _extend(B.receive(rs & 15), rs & 15)
                    pos += 1
        assert B.pos == len(data_r), "bytes left over in an interval"
        pad_bits.append(B.n)
        assert B.acc & ((1 << B.n) - 1) == (1 << B.n) - 1, "padding must be 1-bits"
    nat = np.zeros_like(zz)
    nat[..., ZIGZAG] = zz
    Q = np.stack([P["dqt"][comps[c][3]] for c in comp_of]).reshape(bpm, 64)
    F = (nat * Q).reshape(my, mx, bpm, 8, 8).astype(np.float64)
    s = np.einsum("vy,...vx->...yx", DCT_FLOAT, np.einsum("ux,...vu->...vx", DCT_FLOAT, F)) + 128.0      # [.., y, x]
    s = np.clip(np.rint(s), 0.0, 255.0)        # samples are 8-bit again before up-sampling and colour, as every integer decoder has them

    def plane(blocks):      # [rows, cols, 8, 8] -> [rows * 8, cols * 8]
        return blocks.transpose(0, 2, 1, 3).reshape(blocks.shape[0] * 8, blocks.shape[1] * 8)
    if cn == 1:
        pix = plane(s[:, :, 0]).astype(np.uint8)[:h, :w]
    else:
        if sub == 0:
            Y, Cb, Cr = (plane(s[:, :, k]) for k in range(3))
        else:
            Y = plane(s[:, :, :4].reshape(my, mx, 2, 2, 8, 8).transpose(0, 2, 1, 3, 4, 5).reshape(2 * my, 2 * mx, 8, 8))
            Cb, Cr = (np.repeat(np.repeat(plane(s[:, :, k]), 2, 0), 2, 1) for k in (4, 5))
        R = Y + 1.402 * (Cr - 128)
        G = Y - 0.344136 * (Cb - 128) - 0.714136 * (Cr - 128)
        Bl = Y + 1.772 * (Cb - 128)
        pix = np.clip(np.rint(np.stack([Bl, G, R], -1)), 0, 255).astype(np.uint8)[:h, :w]
    return pix, zz, {"parsed": P, "pad_bits": pad_bits, "sub": sub, "cn": cn}


# ---- the AVI container --------------------------------------------------------------------------------------------------------------
def riff_walk(data):
    """-> (chunks {path: [(offset of the payload, payload)]}, in file order) of a RIFF file; asserts the sizes add up."""
    found = []

    def walk(at, end, path):
        while at < end:
            tag, size = data[at:at + 4], struct.unpack("<I", data[at + 4:at + 8])[0]
            assert at + 8 + size <= end, "a chunk runs past its parent"
            if tag in (b"RIFF", b"LIST"):
                walk(at + 12, at + 8 + size, path + [data[at + 8:at + 12].decode()])
            else:
                found.append(("/".join(path + [tag.decode()]), at + 8, data[at + 8:at + 8 + size]))
            at += 8 + size + (size & 1)
        assert at == end or at == end + 1
    assert data[:4] == b"RIFF" and struct.unpack("<I", data[4:8])[0] == len(data) - 8
    walk(0, len(data), [])
    return found


def check_avi(data, files, w, h, fps):
    """Every 00dc payload is the file handed in, the chunks are even-padded, idx1 points at them, the counts are patched."""
    chunks = riff_walk(data)
    names = [c[0] for c in chunks]
    assert names[:3] == ["AVI /hdrl/avih", "AVI /hdrl/strl/strh", "AVI /hdrl/strl/strf"] and names[-1] == "AVI /idx1"
    frames = [c for c in chunks if c[0] == "AVI /movi/00dc"]
    assert [c[2] for c in frames] == list(files)
    assert all(at % 2 == 0 for _, at, _ in frames)
    avih = struct.unpack("<14I", chunks[0][2])
    assert avih[0] == round(1e6 / fps) and avih[3] & 0x10 and avih[4] == len(files) and avih[6] == 1 and avih[8:10] == (w, h)
    strh = chunks[1][2]
    assert strh[:8] == b"vidsMJPG" and struct.unpack("<I", strh[32:36])[0] == len(files)
    assert abs(struct.unpack("<II", strh[20:28])[1] / struct.unpack("<II", strh[20:28])[0] - fps) < 1e-3
    strf = struct.unpack("<IiiHH4sIiiII", chunks[2][2])
    assert strf[:6] == (40, w, h, 1, 24, b"MJPG")
    idx = chunks[-1][2]
    assert len(idx) == 16 * len(files)
    movi = data.index(b"movi")
    for k, (_, at, payload) in enumerate(frames):
        tag, flags, off, size = struct.unpack("<4sIII", idx[16 * k:16 * k + 16])
        assert tag == b"00dc" and flags == 0x10 and size == len(payload) and movi + off == at - 8
        assert data[movi + off:movi + off + 4] == b"00dc"
