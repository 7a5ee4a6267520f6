"""The JPEG encoder's arithmetic, its host functions and the AVI writer, without a GPU: jpeg_checks restates include/evhip.h
("pictures encoded on the device") and decodes what it wrote; Pillow (libjpeg) is the independent judge where it is installed.

Measured here (CPU), as DESIGN.md section 27 records them:
  * integer DCT against float64: at most 0.5545 on the 2 000 random blocks, 0.6245 on the extremes (bound 1);
  * Pillow's decoder (12.2, libjpeg 6.2) against jpeg_checks.decode on our gray and 4:4:4 files: at most 3 levels (libjpeg's
    integer IDCT and colour rounding), asserted at 4;
  * PSNR against Pillow's encoder at the same tables and subsampling: Pillow leads ours by at most 0.199 dB (video frame, quality
    90, 4:4:4, where it leads the float64-DCT variant by 0.19 dB: the margin is computed per case, that lead plus 0.1 dB);
    sizes: ours / Pillow's at most 1.0561 on these pictures (a restart interval per MCU row costs padding, a marker and a DC
    that starts from 0), asserted at that plus 0.02.
"""
import ctypes as C
import io
import os
import re
import warnings

import numpy as np
import pytest

import jpeg_checks as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MP4 = os.path.join(ROOT, "tests", "golden", "ref_test_video.mp4")
LAYOUTS = [(1, "444"), (3, "444"), (3, "420")]
SIZES = [(1, 1), (7, 9), (8, 8), (9, 7), (16, 16), (17, 9), (33, 17)]
ONES = np.ones((2, 64), np.uint16)
DECODER_GAP = 3          # levels between Pillow's decoder and jpeg_checks.decode, measured on every file of our_files()
SIZE_RATIO = 1.0561      # ours / Pillow's file size, the largest measured in test_quality_against_pillow


def noise(seed, h, w, cn):
    return np.random.default_rng(seed).integers(0, 256, (h, w) if cn == 1 else (h, w, 3), dtype=np.uint8)


def round_trip(zz, cn=1, sub=0, qt=ONES, w=None, h=None):
    """Coefficients [rows, mx, bpm, 64] -> the file, decoded: the coefficients read back must be the ones written."""
    zz = np.asarray(zz)
    mcu = 16 if sub else 8
    w, h = w or zz.shape[1] * mcu, h or zz.shape[0] * mcu
    data = J.encode_coefficients(zz, w, h, cn, sub, qt)
    pix, back, info = J.decode(data)
    assert np.array_equal(back, zz)
    return data, info


# ---- DCT accuracy -------------------------------------------------------------------------------------------------------------
def extreme_blocks():
    y, x = np.mgrid[0:8, 0:8]
    blocks = [np.zeros((8, 8), int), np.full((8, 8), 255), ((x + y) & 1) * 255, ((x + y + 1) & 1) * 255]
    for k in range(64):
        for lo, hi in ((0, 255), (255, 0)):
            b = np.full(64, lo)
            b[k] = hi
            blocks.append(b.reshape(8, 8))
    ramp = np.rint(np.arange(8) * 255 / 7).astype(int)
    blocks += [np.tile(ramp, (8, 1)), np.tile(ramp[::-1], (8, 1)), np.tile(ramp, (8, 1)).T, np.tile(ramp[::-1], (8, 1)).T]
    for v in range(8):                                  # the sign pattern of every basis function: the largest coefficients
        for u in range(8):
            blocks.append((np.outer(J.DCT_FLOAT[v], J.DCT_FLOAT[u]) > 0) * 255)
            blocks.append((np.outer(J.DCT_FLOAT[v], J.DCT_FLOAT[u]) < 0) * 255)
    return np.stack(blocks) - 128


def test_the_integer_dct_is_within_one_of_float64():
    s = np.random.default_rng(1).integers(-128, 128, (2000, 8, 8))
    err = np.abs(J.fdct_int(s) - J.fdct_float(s)).max()
    print("random blocks: %.4f" % err)
    assert err <= 1.0
    e = extreme_blocks()
    err = np.abs(J.fdct_int(e) - J.fdct_float(e)).max()
    print("extremes: %.4f" % err)
    assert err <= 1.0
    # what include/evhip.h says of the sums: both passes fit 32 bits
    a = (np.einsum("ux,...yx->...yu", J.DCT_TABLE, e) + 128) >> 8
    assert np.abs(a).max() <= 11585 and np.abs(J.DCT_TABLE).sum(axis=1).max() * 11585 < 1 << 29


def test_the_table_is_the_one_the_header_prints():
    text = open(os.path.join(ROOT, "include", "evhip.h")).read()
    at = text.index("TRANSFORM: T[u][x]")
    rows = {int(u): [int(v) for v in vals.split()] for u, vals in re.findall(r"u = (\d):((?:\s+-?\d+){8})", text[at:at + 1500])}
    assert sorted(rows) == list(range(8))
    assert np.array_equal(np.array([rows[u] for u in range(8)]), J.DCT_TABLE)


# ---- the entropy layer ----------------------------------------------------------------------------------------------------------
def block(**at):
    z = np.zeros(64, np.int64)
    for k, v in at.items():
        z[int(k[1:])] = v
    return z


def test_crafted_blocks_round_trip():
    blocks = [block(), block(k0=5), block(k63=-3), block(k0=-7, k63=1)]
    for run in (15, 16, 17, 31, 32, 47, 48, 62):
        blocks += [block(**{"k%d" % (run + 1): 2}), block(k0=3, **{"k%d" % (run + 1): -1}), block(k1=1, **{"k%d" % min(run + 2, 63): 5})]
    for zz in blocks:
        round_trip(zz.reshape(1, 1, 1, 64))
    row = np.stack(blocks).reshape(1, len(blocks), 1, 64)                   # and all of them in one interval, in both tables
    round_trip(row)
    colour = np.stack(blocks[:24]).reshape(2, 4, 3, 64)
    round_trip(colour, cn=3)
    round_trip(np.stack(blocks[:24]).reshape(2, 2, 6, 64), cn=3, sub=1)


def test_dc_differences_of_category_11():
    dcs = [-1024, 1016, -1024, 1016, 0, 1016]
    zz = np.zeros((1, len(dcs), 1, 64), np.int64)
    zz[0, :, 0, 0] = dcs
    assert 2040 in np.abs(np.diff(dcs))
    round_trip(zz)
    zz3 = np.zeros((1, len(dcs), 3, 64), np.int64)
    zz3[0, :, :, 0] = np.array(dcs)[:, None]
    round_trip(zz3, cn=3)


def test_the_largest_ac_category_of_8_bit_input():
    F = J.fdct_int(extreme_blocks())
    ac = np.abs(F.reshape(len(F), 64)[:, 1:]).max()
    assert 512 <= ac < 1024, ac                                           # category 10, the last the AC tables have a code for
    for v, u in ((0, 4), (4, 0), (4, 4), (7, 7), (1, 0)):
        pic = ((np.outer(J.DCT_FLOAT[v], J.DCT_FLOAT[u]) > 0) * 255).astype(np.uint8)
        data = J.encode(pic, ONES, "444")
        _, zz, _ = J.decode(data)
        assert np.array_equal(zz, J.coefficients(pic, ONES, "444")) and np.abs(zz[..., 1:]).max() >= 512
    z = block(k0=-1024, k1=1023, k2=-1023, k63=1023)
    round_trip(z.reshape(1, 1, 1, 64))
    round_trip(np.stack([z, -z, z]).reshape(1, 1, 3, 64), cn=3)


def test_stuffed_bytes_and_every_pad_length():
    pic = noise(3, 16, 64, 1)
    data = J.encode(pic, ONES, "444")
    assert data.count(b"\xff\x00") >= 5
    _, zz, _ = J.decode(data)
    assert np.array_equal(zz, J.coefficients(pic, ONES, "444"))
    seen = {}
    for dc in range(-40, 40):
        for a in (0, 1, 2, 5, 9):
            data, info = round_trip(block(k0=dc, k1=a).reshape(1, 1, 1, 64))
            seen.setdefault(info["pad_bits"][0], data)
    assert sorted(seen) == list(range(8)), sorted(seen)                   # intervals ending on a byte and with 1..7 one-bits


def test_restart_markers():
    ten = J.encode(noise(4, 80, 8, 1), J.quant_tables(50), "444")
    P = J.parse(ten)
    assert P["dri"] == 1 and P["rst"] == [0, 1, 2, 3, 4, 5, 6, 7, 0] and len(P["intervals"]) == 10
    one = J.encode(noise(4, 8, 80, 1), J.quant_tables(50), "444")
    P = J.parse(one)
    assert P["dri"] == 10 and P["rst"] == [] and len(P["intervals"]) == 1
    assert not any(bytes([0xFF, 0xD0 + m]) in one[550:] for m in range(8))
    colour = J.parse(J.encode(noise(4, 160, 16, 3), J.quant_tables(50), "420"))
    assert colour["dri"] == 1 and colour["rst"] == [0, 1, 2, 3, 4, 5, 6, 7, 0]
    # every interval stands alone: a picture's row r is the one-row picture of the same pixels
    pic = noise(5, 24, 40, 3)
    whole = J.parse(J.encode(pic, J.quant_tables(75), "444"))["intervals"]
    for r in range(3):
        assert J.parse(J.encode(pic[8 * r:8 * r + 8], J.quant_tables(75), "444"))["intervals"] == [whole[r]]


# ---- geometry -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cn,sub", LAYOUTS)
@pytest.mark.parametrize("w,h", SIZES)
def test_geometry(w, h, cn, sub):
    pic = noise(w * 64 + h, h, w, cn)
    mcu = 16 if sub == "420" else 8
    W, H = -(-w // mcu) * mcu, -(-h // mcu) * mcu
    padded = np.pad(pic, ((0, H - h), (0, W - w)) + (((0, 0),) if cn == 3 else ()), mode="edge")
    qt = J.quant_tables(90)
    zz = J.coefficients(pic, qt, sub)
    assert zz.shape == (H // mcu, W // mcu, {(1, "444"): 1, (3, "444"): 3, (3, "420"): 6}[(cn, sub)], 64)
    assert np.array_equal(zz, J.coefficients(padded, qt, sub))             # pixels past the edge repeat it
    data = J.encode(pic, qt, sub)
    pix, back, info = J.decode(data)
    assert pix.shape == pic.shape and np.array_equal(back, zz)
    assert len(data) <= J.bound(w, h, cn, J.SUBSAMPLINGS[sub])
    for v in (0, 1, 127, 128, 200, 255):                                   # a flat picture comes back as it went in
        flat = np.full(pic.shape, v, np.uint8)
        got, zz, _ = J.decode(J.encode(flat, qt, sub))
        assert np.all(got == v), (v, np.unique(got))
        assert not zz[..., 1:].any()


def test_gray_stays_gray_in_colour():
    v = np.arange(256)
    c = J.ycc(np.stack([v, v, v], -1))
    assert np.array_equal(c[:, 0], v) and np.all(c[:, 1:] == 128)
    every = np.stack(np.meshgrid([0, 1, 127, 128, 254, 255], [0, 1, 127, 128, 254, 255], [0, 1, 127, 128, 254, 255]), -1).reshape(-1, 3)
    assert J.ycc(every).min() >= 0 and J.ycc(every).max() <= 255


# ---- tables and host functions ----------------------------------------------------------------------------------------------------
def test_quant_tables():
    from evenvizion_amd.pictures import quant_tables
    for q in (1, 10, 49, 50, 51, 75, 90, 100):
        s = 5000 // q if q < 50 else 200 - 2 * q
        want = [[min(max((int(b) * s + 50) // 100, 1), 255) for b in base] for base in (J.K1, J.K2)]
        got = quant_tables(q)
        assert got.dtype == np.uint16 and got.shape == (2, 64) and got.tolist() == want, q
    assert quant_tables(50).tolist() == [J.K1.tolist(), J.K2.tolist()]
    assert np.all(quant_tables(100) == 1) and np.all(quant_tables(1) == 255)
    assert quant_tables(75)[0, :8].tolist() == [8, 6, 5, 8, 12, 20, 26, 31]
    for bad in (0, 101):
        with pytest.raises(ValueError):
            quant_tables(bad)


def lib():
    from evenvizion_amd import _lib
    _lib.build()
    return _lib


@pytest.mark.parametrize("cn,sub", LAYOUTS)
def test_bound_holds_for_noise_under_all_ones_tables(cn, sub):
    L = lib()
    for w, h in SIZES + [(64, 48)]:
        assert L.jpeg_bound(w, h, cn, sub) == J.bound(w, h, cn, J.SUBSAMPLINGS[sub])
        for seed in range(3):
            data = J.encode(noise(seed, h, w, cn), ONES, sub)
            assert len(data) <= L.jpeg_bound(w, h, cn, sub)
    # the largest block the restatement can be handed stays inside the per-block figure
    z = np.full(64, 1023)
    z[0] = -1024
    z[1::2] = -1023
    y = -z
    y[0] = 1016                                                            # the largest difference: category 11
    data, _ = round_trip(np.stack([z, y]).reshape(1, 2, 1, 64))
    assert (len(data) - 550 - 2) * 8 <= 2 * 2 * J.BLOCK_BITS + 16
    for bad in ((0, 8, 1, 0), (8, 65536, 1, 0), (8, 8, 2, 0), (8, 8, 1, 1), (8, 8, 3, 2)):
        assert L.load().evh_jpeg_bound(*bad) == -1


def test_header_is_the_restatement_byte_for_byte():
    L = lib()
    for qt in (J.quant_tables(75), ONES, J.quant_tables(10)):
        for cn, sub in LAYOUTS:
            for w, h in SIZES + [(65535, 65535), (400, 224)]:
                head = L.jpeg_header(w, h, cn, qt, sub)
                assert head == J.header(w, h, cn, J.SUBSAMPLINGS[sub], qt)
                assert len(head) == (550 if cn == 1 else 629)
    fn, q, out = L.load().evh_jpeg_header, np.ascontiguousarray(J.quant_tables(75)), np.full(700, 0xEE, np.uint8)
    qp, op = q.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    bad_q = q.copy()
    bad_q[1, 0] = 0
    for args in ((0, 8, 3, 1, qp, op, 700), (8, 8, 1, 1, qp, op, 700), (8, 8, 3, 1, None, op, 700), (8, 8, 3, 1, qp, None, 700),
                 (8, 8, 3, 1, qp, op, 628), (8, 8, 1, 0, qp, op, 549), (8, 8, 3, 1, bad_q.ctypes.data_as(C.c_void_p), op, 700)):
        assert fn(*args) == -1 and np.all(out == 0xEE), args[:4]
    assert fn(8, 8, 3, 1, qp, op, 629) == 629 and np.all(out[629:] == 0xEE)


def test_ctypes_table_matches_the_declarations():
    from evenvizion_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "evhip.h")).read(), flags=re.S)
    kinds = {"int": C.c_int, "int64_t": C.c_int64, "double": C.c_double}
    found = 0
    for ret, name, args in re.findall(r"\b(int64_t|int)\s+(evh_jpeg_\w+)\s*\(([^)]*)\)\s*;", text):
        want = [C.c_void_p if "*" in a else kinds[a.split()[-2] if len(a.split()) > 1 else a.split()[0]] for a in args.split(",")]
        assert _lib.SIGNATURES[name] == (kinds[ret], want), name
        found += 1
    assert found == 3
    assert (_lib.JPEG_444, _lib.JPEG_420) == (0, 1) and re.search(r"EVH_JPEG_444 = 0, EVH_JPEG_420 = 1", text)


def test_mjpeg_avi_writer(tmp_path):
    from evenvizion_amd.pictures import MjpegAviWriter
    files = [J.encode(noise(k, 16, 24, 3), J.quant_tables(50 + 10 * k), "420") for k in range(5)]
    files[2] += b"\x00" if len(files[2]) % 2 == 0 else b""                # an odd and an even length among them
    files[3] += b"\x00" if len(files[3]) % 2 == 1 else b""
    assert {len(f) % 2 for f in files} == {0, 1}
    path = str(tmp_path / "a.avi")
    with MjpegAviWriter(path, 24, 16, 12.5) as wr:
        for f in files:
            wr.write(f)
    J.check_avi(open(path, "rb").read(), files, 24, 16, 12.5)
    empty = str(tmp_path / "b.avi")
    MjpegAviWriter(empty, 8, 8, 25).close()
    J.check_avi(open(empty, "rb").read(), [], 8, 8, 25)
    wr = MjpegAviWriter(str(tmp_path / "c.avi"), 8, 8, 25)
    wr.size = wr.LIMIT - 100                                               # as if 2 GiB had been written
    with pytest.raises(ValueError):
        wr.write(files[0])
    wr.close()
    for bad in ((0, 8, 25), (8, 65536, 25), (8, 8, 0)):
        with pytest.raises(ValueError):
            MjpegAviWriter(str(tmp_path / "d.avi"), *bad)


# ---- the independent judge --------------------------------------------------------------------------------------------------------
def pil_pixels(data):
    from PIL import Image
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        im = Image.open(io.BytesIO(data))
        im.load()
    a = np.asarray(im)
    return a if a.ndim == 2 else a[..., ::-1]


def our_files():
    for w, h in SIZES + [(80, 8), (8, 80), (64, 48)]:
        for cn, sub in LAYOUTS:
            pic = noise(w + h, h, w, cn)
            for qt in (ONES, J.quant_tables(50), J.quant_tables(90)):
                yield cn, sub, pic, J.encode(pic, qt, sub)
            smooth = np.clip(np.add.outer(np.arange(h) * 3, np.arange(w) * 2)[..., None] + np.array([0, 40, 90]), 0, 255).astype(np.uint8)
            yield cn, sub, smooth[..., 0] if cn == 1 else smooth, J.encode(smooth[..., 0] if cn == 1 else smooth, J.quant_tables(75), sub)


def test_pillow_decodes_every_file():
    pytest.importorskip("PIL")
    worst = 0
    for cn, sub, pic, data in our_files():
        got = pil_pixels(data)
        assert got.shape == pic.shape
        if sub == "444":
            own, _, _ = J.decode(data)
            worst = max(worst, int(np.abs(got.astype(int) - own.astype(int)).max()))
    print("Pillow's decoder against jpeg_checks.decode: %d levels" % worst)
    assert worst <= DECODER_GAP + 1


def test_pillow_writes_the_same_standard_tables():
    pytest.importorskip("PIL")
    from PIL import Image
    from evenvizion_amd.pictures import quant_tables
    im = Image.fromarray(noise(1, 16, 16, 3))
    for q in (50, 75, 90):
        b = io.BytesIO()
        im.save(b, "JPEG", quality=q, optimize=False, subsampling=2)
        P = J.parse(b.getvalue())
        assert np.array_equal(np.stack([P["dqt"][0], P["dqt"][1]]), quant_tables(q))
        ours = J.parse(J.encode(np.asarray(im), quant_tables(q), "420"))
        assert P["dht_raw"] == ours["dht_raw"] and sorted(ours["dht_raw"]) == [(0, 0), (0, 1), (1, 0), (1, 1)]
        assert ours["dht_raw"][(1, 0)] == (J.AC_BITS[0], J.AC_VALS[0]) and ours["dht_raw"][(1, 1)] == (J.AC_BITS[1], J.AC_VALS[1])


def quality_pictures():
    from evenvizion_amd import capture, synthetic
    rng = np.random.default_rng(9)
    g = rng.integers(0, 256, (48 + 8, 64 + 8, 3)).astype(np.float64)
    k = np.ones(9) / 9
    for axis in (0, 1):
        g = np.apply_along_axis(lambda v: np.convolve(v, k, mode="valid"), axis, g)
    filtered = np.clip((g - 128) * 3 + 128, 0, 255).astype(np.uint8)
    frame = synthetic.make_stream(3, 1, 96, 64)[0][0]
    colour = np.stack([frame, np.roll(frame, 3, 1), 255 - frame], -1)
    ok, video = capture.VideoCapture(MP4).read()
    assert ok
    return {"filtered noise": filtered, "synthetic frame": colour, "video frame": np.ascontiguousarray(video[100:260, 200:440])}


def psnr(a, b):
    return 10 * np.log10(255.0 ** 2 / np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))


def test_quality_against_pillow():
    """Ours may fall below Pillow's encoder by Pillow's lead over the ideal-arithmetic variant (float64 DCT, our sampling) plus 0.1 dB."""
    pytest.importorskip("PIL")
    from PIL import Image
    from evenvizion_amd.pictures import quant_tables
    worst_ratio, worst_lead = 0.0, -99.0
    for name, pic in quality_pictures().items():
        assert pic.shape[0] >= 48 and pic.shape[1] >= 64
        for q in (50, 75, 90):
            for sub in ("420", "444"):
                b = io.BytesIO()
                Image.fromarray(np.ascontiguousarray(pic[..., ::-1])).save(b, "JPEG", quality=q, optimize=False, subsampling=2 if sub == "420" else 0)
                theirs = b.getvalue()
                ours, ideal = J.encode(pic, quant_tables(q), sub), J.encode(pic, quant_tables(q), sub, dct=J.fdct_ideal)
                p_theirs, p_ours, p_ideal = (psnr(pil_pixels(f), pic) for f in (theirs, ours, ideal))
                margin = max(0.0, p_theirs - p_ideal) + 0.1
                ratio = len(ours) / len(theirs)
                print("%-16s q%d %s: Pillow %.2f dB %d B, ours %.2f dB %d B (x%.3f), ideal %.2f dB, margin %.2f"
                      % (name, q, sub, p_theirs, len(theirs), p_ours, len(ours), ratio, p_ideal, margin))
                assert p_ours >= p_theirs - margin, (name, q, sub)
                worst_ratio, worst_lead = max(worst_ratio, ratio), max(worst_lead, p_theirs - p_ours)
    print("largest size ratio %.4f, Pillow's largest lead %.3f dB" % (worst_ratio, worst_lead))
    assert worst_ratio <= SIZE_RATIO + 0.02
