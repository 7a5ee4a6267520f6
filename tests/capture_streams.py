"""Stream construction for tests/test_capture_hostile.py (a helper module, not a test file; standard library only).

    Mp4File / list_samples / split_nals   an ISO-BMFF reader of its own (stsz, stco/co64, stsc, avcC), independent of evc_mp4.cpp
    write_mp4                             a minimal writer: ftyp, moov/trak/mdia/minf/stbl (stsd avc1+avcC, stts, stsc, stsz, stco), mdat
    BitWriter / BitReader                 u(n), ue(v), se(v); rbsp_to_nal / nal_to_rbsp add and remove emulation prevention
    edit_sps / edit_pps                   parse a parameter set and re-emit it with chosen fields changed
    CabacEncoder / ipcm_stream            an arithmetic *encoder* by ITU-T Rec. H.264 clause 9.3.4 and a writer of pictures whose
                                          macroblocks are all I_PCM: the decode of such a stream is the planes themselves

Clause numbers refer to ITU-T Rec. H.264; box names to ISO/IEC 14496-12 and -15.
"""
import struct

# ------------------------------------------------------------------------------------------------------------------ bits


class BitWriter:
    def __init__(self):
        self.buf, self.acc, self.nacc = bytearray(), 0, 0      # whole bytes; the bits of the unfinished byte and their number

    def u(self, n, v):
        assert 0 <= v < (1 << n) if n else v == 0, (n, v)
        self.acc, self.nacc = (self.acc << n) | v, self.nacc + n
        while self.nacc >= 8:
            self.nacc -= 8
            self.buf.append((self.acc >> self.nacc) & 255)
        self.acc &= (1 << self.nacc) - 1
        return self

    def put_bytes(self, data):
        assert self.aligned()
        self.buf += data
        return self

    def ue(self, v):                                     # 9.1
        assert v >= 0
        n = (v + 1).bit_length() - 1
        self.u(n, 0)
        self.u(n + 1, v + 1)
        return self

    def se(self, v):                                     # 9.1.1
        return self.ue(2 * v - 1 if v > 0 else -2 * v)

    def raw(self, bits):
        for b in bits:
            self.u(1, b)
        return self

    def aligned(self):
        return self.nacc == 0

    def trailing(self):                                  # 7.3.2.11 rbsp_trailing_bits
        self.u(1, 1)
        while not self.aligned():
            self.u(1, 0)
        return self

    def bytes(self):
        assert self.aligned()
        return bytes(self.buf)


class BitReader:
    def __init__(self, data):
        self.d = data
        self.pos = 0
        self.n = len(data) * 8

    def u(self, n):
        v = 0
        for _ in range(n):
            if self.pos >= self.n:
                raise ValueError("read past the end of the RBSP")
            v = (v << 1) | ((self.d[self.pos >> 3] >> (7 - (self.pos & 7))) & 1)
            self.pos += 1
        return v

    def ue(self):
        z = 0
        while self.u(1) == 0:
            z += 1
            if z > 32:
                raise ValueError("Exp-Golomb prefix too long")
        return (1 << z) - 1 + self.u(z) if z else 0

    def se(self):
        k = self.ue()
        return (k + 1) >> 1 if k & 1 else -(k >> 1)

    def stop_bit_pos(self):
        """position of rbsp_stop_one_bit: the last 1 bit of the payload"""
        p = self.n
        while p > 0 and not (self.d[(p - 1) >> 3] >> (7 - ((p - 1) & 7))) & 1:
            p -= 1
        if p == 0:
            raise ValueError("no rbsp_stop_one_bit")
        return p - 1

    def more_rbsp_data(self):
        return self.pos < self.stop_bit_pos()

    def rest(self):
        """the bits from here up to (not including) rbsp_stop_one_bit"""
        end = self.stop_bit_pos()
        return [self.u(1) for _ in range(end - self.pos)]


def nal_to_rbsp(payload):
    """7.4.1: drops emulation_prevention_three_byte (the NAL header byte is not part of `payload`)"""
    out, zeros = bytearray(), 0
    for b in payload:
        if zeros >= 2 and b == 3:
            zeros = 0
            continue
        out.append(b)
        zeros = zeros + 1 if b == 0 else 0
    return bytes(out)


def rbsp_to_nal(header, rbsp):
    """7.4.1: NAL header byte + payload with 00 00 03 before any 00 00 0x (x <= 3); a final 00 gets a 03 behind it"""
    out, zeros = bytearray([header]), 0
    for b in rbsp:
        if zeros >= 2 and b <= 3:
            out.append(3)
            zeros = 0
        out.append(b)
        zeros = zeros + 1 if b == 0 else 0
    if rbsp and rbsp[-1] == 0:
        out.append(3)
    return bytes(out)


# ---------------------------------------------------------------------------------------------------------- parameter sets
_HIGH_PROFILES = (100, 110, 122, 244, 44, 83, 86, 118, 128, 138, 139, 134, 135)


def parse_sps(nal):
    """-> dict of the fields up to the cropping offsets, plus "rest": the bits behind them (VUI flag and VUI) verbatim"""
    assert nal[0] & 31 == 7
    b = BitReader(nal_to_rbsp(nal[1:]))
    s = {"nal_header": nal[0], "profile_idc": b.u(8), "constraint_flags": b.u(8), "level_idc": b.u(8), "sps_id": b.ue()}
    s["high"] = s["profile_idc"] in _HIGH_PROFILES
    if s["high"]:
        s["chroma_format_idc"] = b.ue()
        if s["chroma_format_idc"] == 3:
            raise NotImplementedError("4:4:4")
        s["bit_depth_luma_minus8"], s["bit_depth_chroma_minus8"] = b.ue(), b.ue()
        s["transform_bypass"] = b.u(1)
        if b.u(1):
            raise NotImplementedError("seq_scaling_matrix_present_flag")
    s["log2_max_frame_num_minus4"] = b.ue()
    s["poc_type"] = b.ue()
    if s["poc_type"] == 0:
        s["log2_max_poc_lsb_minus4"] = b.ue()
    elif s["poc_type"] != 2:
        raise NotImplementedError("pic_order_cnt_type 1")
    s["max_num_ref_frames"] = b.ue()
    s["gaps_in_frame_num_allowed"] = b.u(1)
    s["mb_w"], s["mb_h"] = b.ue() + 1, b.ue() + 1
    s["frame_mbs_only"] = b.u(1)
    if not s["frame_mbs_only"]:
        raise NotImplementedError("interlace")
    s["direct_8x8_inference"] = b.u(1)
    s["crop"] = (b.ue(), b.ue(), b.ue(), b.ue()) if b.u(1) else None      # left, right, top, bottom in crop units
    s["rest"] = b.rest()
    return s


def emit_sps(s):
    w = BitWriter()
    w.u(8, s["profile_idc"]).u(8, s["constraint_flags"]).u(8, s["level_idc"]).ue(s["sps_id"])
    if s["high"]:
        w.ue(s["chroma_format_idc"]).ue(s["bit_depth_luma_minus8"]).ue(s["bit_depth_chroma_minus8"])
        w.u(1, s["transform_bypass"]).u(1, 0)
    w.ue(s["log2_max_frame_num_minus4"]).ue(s["poc_type"])
    if s["poc_type"] == 0:
        w.ue(s["log2_max_poc_lsb_minus4"])
    w.ue(s["max_num_ref_frames"]).u(1, s["gaps_in_frame_num_allowed"]).ue(s["mb_w"] - 1).ue(s["mb_h"] - 1)
    w.u(1, 1).u(1, s["direct_8x8_inference"])
    if s["crop"] is None:
        w.u(1, 0)
    else:
        w.u(1, 1)
        for v in s["crop"]:
            w.ue(v)
    w.raw(s["rest"]).trailing()
    return rbsp_to_nal(s["nal_header"], w.bytes())


def edit_sps(nal, **fields):
    """the SPS `nal` with the named fields of parse_sps() replaced (mb_w, mb_h, crop, max_num_ref_frames,
    log2_max_frame_num_minus4, sps_id, ...); with no field the result decodes to the same parameter set"""
    s = parse_sps(nal)
    for k, v in fields.items():
        assert k in s, k
        s[k] = v
    return emit_sps(s)


def parse_pps(nal):
    assert nal[0] & 31 == 8
    b = BitReader(nal_to_rbsp(nal[1:]))
    p = {"nal_header": nal[0], "pps_id": b.ue(), "sps_id": b.ue(), "cabac": b.u(1), "bottom_field_pic_order": b.u(1)}
    if b.ue() != 0:
        raise NotImplementedError("slice groups")
    p["num_ref_idx_default"] = (b.ue() + 1, b.ue() + 1)
    p["weighted_pred"], p["weighted_bipred_idc"] = b.u(1), b.u(2)
    p["pic_init_qp_minus26"], p["pic_init_qs_minus26"], p["chroma_qp_index_offset"] = b.se(), b.se(), b.se()
    p["deblocking_control"], p["constrained_intra_pred"], p["redundant_pic_cnt"] = b.u(1), b.u(1), b.u(1)
    p["extension"] = b.more_rbsp_data()
    p["transform_8x8_mode"], p["second_chroma_qp_index_offset"] = 0, p["chroma_qp_index_offset"]
    if p["extension"]:
        p["transform_8x8_mode"] = b.u(1)
        if b.u(1):
            raise NotImplementedError("pic_scaling_matrix_present_flag")
        p["second_chroma_qp_index_offset"] = b.se()
    return p


def emit_pps(p):
    w = BitWriter()
    w.ue(p["pps_id"]).ue(p["sps_id"]).u(1, p["cabac"]).u(1, p["bottom_field_pic_order"]).ue(0)
    w.ue(p["num_ref_idx_default"][0] - 1).ue(p["num_ref_idx_default"][1] - 1)
    w.u(1, p["weighted_pred"]).u(2, p["weighted_bipred_idc"])
    w.se(p["pic_init_qp_minus26"]).se(p["pic_init_qs_minus26"]).se(p["chroma_qp_index_offset"])
    w.u(1, p["deblocking_control"]).u(1, p["constrained_intra_pred"]).u(1, p["redundant_pic_cnt"])
    if p["extension"] or p["transform_8x8_mode"] or p["second_chroma_qp_index_offset"] != p["chroma_qp_index_offset"]:
        w.u(1, p["transform_8x8_mode"]).u(1, 0).se(p["second_chroma_qp_index_offset"])
    w.trailing()
    return rbsp_to_nal(p["nal_header"], w.bytes())


def edit_pps(nal, **fields):
    """the PPS `nal` with the named fields of parse_pps() replaced (num_ref_idx_default, weighted_pred, weighted_bipred_idc,
    transform_8x8_mode, ...)"""
    p = parse_pps(nal)
    for k, v in fields.items():
        assert k in p, k
        p[k] = v
    return emit_pps(p)


def slice_type_of(nal):
    """'P' | 'B' | 'I' of a slice NAL unit (7.3.3: first_mb_in_slice, slice_type)"""
    b = BitReader(nal_to_rbsp(nal[1:16]))
    b.ue()
    return "PBI"[b.ue() % 5]


# -------------------------------------------------------------------------------------------------------------- MP4 reader
_CONTAINERS = (b"moov", b"trak", b"mdia", b"minf", b"stbl", b"edts", b"dinf")


def boxes(data, start=0, end=None):
    """[(type, box offset, payload offset, end offset)] of the boxes in data[start:end]"""
    end = len(data) if end is None else end
    out, o = [], start
    while o + 8 <= end:
        size, tp = struct.unpack(">I4s", data[o:o + 8])
        hdr = 8
        if size == 1:
            size, hdr = struct.unpack(">Q", data[o + 8:o + 16])[0], 16
        elif size == 0:
            size = end - o
        if size < hdr or o + size > end:
            raise ValueError("box %r of %d bytes does not fit its parent" % (tp, size))
        out.append((tp, o, o + hdr, o + size))
        o += size
    return out


def find_box(data, path, start=0, end=None):
    """(box offset, payload offset, end offset) of the first box at `path`, e.g. "moov/trak/mdia/minf/stbl/stsz" """
    tp, _, rest = path.partition("/")
    for t, o, body, e in boxes(data, start, end):
        if t == tp.encode():
            return find_box(data, rest, body, e) if rest else (o, body, e)
    raise KeyError(path)


def all_boxes(data, start=0, end=None, depth=0):
    """every box of the file, containers descended into: [(type, box offset, payload offset, end offset, depth)]"""
    out = []
    for t, o, body, e in boxes(data, start, end):
        out.append((t, o, body, e, depth))
        if t in _CONTAINERS:
            out += all_boxes(data, body, e, depth + 1)
    return out


class Mp4File:
    """The video track of an MP4: parameter sets, NAL length size, samples as (offset, size)."""

    def __init__(self, data):
        self.data = data
        stbl = "moov/trak/mdia/minf/stbl/"
        _, body, end = find_box(data, stbl + "stsd")
        entry = body + 8
        esz, etp = struct.unpack(">I4s", data[entry:entry + 8])
        assert etp in (b"avc1", b"avc3"), etp
        self.width, self.height = struct.unpack(">HH", data[entry + 32:entry + 36])
        _, a, _ = find_box(data, "avcC", entry + 86, entry + esz)
        assert data[a] == 1
        self.nal_length_size = (data[a + 4] & 3) + 1
        self.sps, self.pps = [], []
        n, a = data[a + 5] & 31, a + 6
        for _ in range(n):
            ln = struct.unpack(">H", data[a:a + 2])[0]
            self.sps.append(data[a + 2:a + 2 + ln])
            a += 2 + ln
        n, a = data[a], a + 1
        for _ in range(n):
            ln = struct.unpack(">H", data[a:a + 2])[0]
            self.pps.append(data[a + 2:a + 2 + ln])
            a += 2 + ln
        _, body, _ = find_box(data, stbl + "stsz")
        fixed, count = struct.unpack(">II", data[body + 4:body + 12])
        sizes = [fixed] * count if fixed else list(struct.unpack(">%dI" % count, data[body + 12:body + 12 + 4 * count]))
        try:
            _, body, _ = find_box(data, stbl + "stco")
            n = struct.unpack(">I", data[body + 4:body + 8])[0]
            chunks = list(struct.unpack(">%dI" % n, data[body + 8:body + 8 + 4 * n]))
        except KeyError:
            _, body, _ = find_box(data, stbl + "co64")
            n = struct.unpack(">I", data[body + 4:body + 8])[0]
            chunks = list(struct.unpack(">%dQ" % n, data[body + 8:body + 8 + 8 * n]))
        _, body, _ = find_box(data, stbl + "stsc")
        n = struct.unpack(">I", data[body + 4:body + 8])[0]
        runs = [struct.unpack(">III", data[body + 8 + 12 * i:body + 20 + 12 * i]) for i in range(n)]
        self.samples, s = [], 0
        for i, (first, per, _desc) in enumerate(runs):
            last = runs[i + 1][0] - 1 if i + 1 < n else len(chunks)
            for c in range(first, last + 1):
                o = chunks[c - 1]
                for _ in range(per):
                    if s == count:
                        break
                    self.samples.append((o, sizes[s]))
                    o += sizes[s]
                    s += 1
        assert s == count, (s, count)

    def sample_nals(self, i):
        o, n = self.samples[i]
        return split_nals(self.data[o:o + n], self.nal_length_size)


def list_samples(data):
    return Mp4File(data).samples


def split_nals(sample, length_size):
    out, o = [], 0
    while o < len(sample):
        ln = int.from_bytes(sample[o:o + length_size], "big")
        o += length_size
        if o + ln > len(sample):
            raise ValueError("a NAL unit of %d bytes overruns its sample" % ln)
        out.append(sample[o:o + ln])
        o += ln
    return out


# -------------------------------------------------------------------------------------------------------------- MP4 writer
def box(tp, *payload):
    body = b"".join(payload)
    return struct.pack(">I4s", 8 + len(body), tp) + body


def full(tp, version, flags, *payload):
    return box(tp, struct.pack(">I", (version << 24) | flags), *payload)


def join_nals(nals, length_size=4):
    return b"".join(len(n).to_bytes(length_size, "big") + n for n in nals)


def write_mp4(samples, sps, pps, width, height, length_size=4, timescale=15360, delta=512, raw_samples=False, ctts=None, elst=None,
              co64=False):
    """samples: a list of samples, each a list of NAL units (or, with raw_samples, the bytes of the sample as they stand);
    sps / pps: the parameter sets of avcC.  One chunk holds all samples.  ctts: [(count, offset)], elst: [(segment_duration,
    media_time)] (version 0, media_time signed) are written when given; co64 writes the chunk offset as 64 bits."""
    blobs = [s if raw_samples else join_nals(s, length_size) for s in samples]
    avcc = bytes([1, sps[0][1], sps[0][2], sps[0][3], 0xFC | (length_size - 1), 0xE0 | len(sps)])
    avcc += b"".join(struct.pack(">H", len(s)) + s for s in sps) + bytes([len(pps)])
    avcc += b"".join(struct.pack(">H", len(p)) + p for p in pps)
    avc1 = box(b"avc1", bytes(6), struct.pack(">H", 1), bytes(16), struct.pack(">HH", width, height),
               struct.pack(">II", 0x480000, 0x480000), bytes(4), struct.pack(">H", 1), bytes(32), struct.pack(">Hh", 24, -1),
               box(b"avcC", avcc))
    assert len(avc1) == 86 + 8 + len(avcc)
    duration = delta * len(blobs)

    def moov(first_offset):
        stbl = [full(b"stsd", 0, 0, struct.pack(">I", 1), avc1),
                full(b"stts", 0, 0, struct.pack(">III", 1, len(blobs), delta))]
        if ctts is not None:
            stbl.append(full(b"ctts", 0, 0, struct.pack(">I", len(ctts)), *[struct.pack(">II", c, o) for c, o in ctts]))
        stbl += [full(b"stsc", 0, 0, struct.pack(">IIII", 1, 1, len(blobs), 1)),
                 full(b"stsz", 0, 0, struct.pack(">II", 0, len(blobs)), *[struct.pack(">I", len(b)) for b in blobs]),
                 full(b"co64", 0, 0, struct.pack(">IQ", 1, first_offset)) if co64 else
                 full(b"stco", 0, 0, struct.pack(">II", 1, first_offset))]
        minf = box(b"minf", full(b"vmhd", 0, 1, bytes(8)), box(b"stbl", *stbl))
        mdia = box(b"mdia", full(b"mdhd", 0, 0, struct.pack(">IIIIHH", 0, 0, timescale, duration, 0x55C4, 0)),
                   full(b"hdlr", 0, 0, bytes(4), b"vide", bytes(12), b"video\0"), minf)
        trak = [full(b"tkhd", 0, 3, struct.pack(">IIIII", 0, 0, 1, 0, duration), bytes(8 + 8), bytes(36),
                     struct.pack(">II", width << 16, height << 16))]
        if elst is not None:
            trak.append(box(b"edts", full(b"elst", 0, 0, struct.pack(">I", len(elst)),
                                          *[struct.pack(">IiI", d, t, 0x10000) for d, t in elst])))
        trak.append(mdia)
        mvhd = full(b"mvhd", 0, 0, struct.pack(">IIII", 0, 0, timescale, duration), bytes(80))
        return box(b"moov", mvhd, box(b"trak", *trak))

    ftyp = box(b"ftyp", b"isom", struct.pack(">I", 512), b"isomavc1")
    first = len(ftyp) + len(moov(0)) + 8
    return ftyp + moov(first) + box(b"mdat", *blobs)


# ------------------------------------------------------------------------------------------------------- CABAC encoder
# Table 9-44 rangeTabLPS and Table 9-45 transIdxLPS (transIdxMPS is min(pStateIdx + 1, 62)); data of the Recommendation.
RANGE_TAB_LPS = (
    (128, 176, 208, 240), (128, 167, 197, 227), (128, 158, 187, 216), (123, 150, 178, 205), (116, 142, 169, 195),
    (111, 135, 160, 185), (105, 128, 152, 175), (100, 122, 144, 166), (95, 116, 137, 158), (90, 110, 130, 150),
    (85, 104, 123, 142), (81, 99, 117, 135), (77, 94, 111, 128), (73, 89, 105, 122), (69, 85, 100, 116),
    (66, 80, 95, 110), (62, 76, 90, 104), (59, 72, 86, 99), (56, 69, 81, 94), (53, 65, 77, 89),
    (51, 62, 73, 85), (48, 59, 69, 80), (46, 56, 66, 76), (43, 53, 63, 72), (41, 50, 59, 69),
    (39, 48, 56, 65), (37, 45, 54, 62), (35, 43, 51, 59), (33, 41, 48, 56), (32, 39, 46, 53),
    (30, 37, 43, 50), (29, 35, 41, 48), (27, 33, 39, 45), (26, 31, 37, 43), (24, 30, 35, 41),
    (23, 28, 33, 39), (22, 27, 32, 37), (21, 26, 30, 35), (20, 24, 29, 33), (19, 23, 27, 31),
    (18, 22, 26, 30), (17, 21, 25, 28), (16, 20, 23, 27), (15, 19, 22, 25), (14, 18, 21, 24),
    (14, 17, 20, 23), (13, 16, 19, 22), (12, 15, 18, 21), (12, 14, 17, 20), (11, 14, 16, 19),
    (11, 13, 15, 18), (10, 12, 15, 17), (10, 12, 14, 16), (9, 11, 13, 15), (9, 11, 12, 14),
    (8, 10, 12, 14), (8, 9, 11, 13), (7, 9, 11, 12), (7, 9, 10, 12), (7, 8, 10, 11),
    (6, 8, 9, 11), (6, 7, 9, 10), (6, 7, 8, 9), (2, 2, 2, 2))
TRANS_IDX_LPS = (0, 0, 1, 2, 2, 4, 4, 5, 6, 7, 8, 9, 9, 11, 11, 12, 13, 13, 15, 15, 16, 16, 18, 18, 19, 19, 21, 21, 22, 22, 23, 24,
                 24, 25, 26, 26, 27, 27, 28, 29, 29, 30, 30, 30, 31, 32, 32, 33, 33, 33, 34, 34, 35, 35, 35, 36, 36, 36, 37, 37,
                 37, 38, 38, 63)
# Table 9-12: (m, n) of ctxIdx 3, 4, 5 -- the first bin of mb_type in I slices
MB_TYPE_I_INIT = {3: (20, -15), 4: (2, 54), 5: (3, 74)}


class CabacEncoder:
    """9.3.4: the arithmetic encoding process, appending bits to a BitWriter.  Only what an all-I_PCM slice needs is here:
    EncodeDecision (9.3.4.2) for the first bin of mb_type, EncodeTerminate / EncodeFlush (9.3.4.5), RenormE and PutBit
    (9.3.4.3), and the initialisations of 9.3.1.1 (context variables) and 9.3.4.1 (engine)."""

    def __init__(self, out, slice_qp):
        self.out = out
        self.ctx = {}
        for idx, (m, n) in MB_TYPE_I_INIT.items():       # 9.3.1.1
            pre = min(max(((m * min(max(slice_qp, 0), 51)) >> 4) + n, 1), 126)
            self.ctx[idx] = [63 - pre, 0] if pre <= 63 else [pre - 64, 1]      # [pStateIdx, valMPS]
        self.init_engine()

    def init_engine(self):                               # 9.3.4.1
        self.low, self.range, self.first_bit, self.outstanding = 0, 510, True, 0

    def put_bit(self, b):                                # 9.3.4.3, Figure 9-10
        if self.first_bit:
            self.first_bit = False
        else:
            self.out.u(1, b)
        while self.outstanding > 0:
            self.out.u(1, 1 - b)
            self.outstanding -= 1

    def renorm(self):                                    # 9.3.4.3, Figure 9-9
        while self.range < 256:
            if self.low < 256:
                self.put_bit(0)
            elif self.low >= 512:
                self.low -= 512
                self.put_bit(1)
            else:
                self.low -= 256
                self.outstanding += 1
            self.range <<= 1
            self.low <<= 1

    def decision(self, ctx_idx, bin_val):                # 9.3.4.2, Figure 9-8
        st = self.ctx[ctx_idx]
        r_lps = RANGE_TAB_LPS[st[0]][(self.range >> 6) & 3]
        self.range -= r_lps
        if bin_val != st[1]:
            self.low += self.range
            self.range = r_lps
            if st[0] == 0:
                st[1] = 1 - st[1]
            st[0] = TRANS_IDX_LPS[st[0]]
        else:
            st[0] = min(st[0] + 1, 62)
        self.renorm()

    def terminate(self, bin_val):                        # 9.3.4.5, Figure 9-12
        self.range -= 2
        if bin_val:
            self.low += self.range
            self.flush()
        else:
            self.renorm()

    def flush(self):                                     # 9.3.4.5, Figure 9-13
        self.range = 2
        self.renorm()
        self.put_bit((self.low >> 9) & 1)
        self.out.u(2, ((self.low >> 7) & 3) | 1)          # the last bit written is rbsp_stop_one_bit at the end of a slice


def ipcm_sps(mb_w, mb_h, crop=None, sps_id=0):
    """A Main-profile SPS: pic_order_cnt_type 2, one reference frame, frame_mbs_only; crop = (left, right, top, bottom) in
    crop units (two luma samples each in 4:2:0), or None."""
    w = BitWriter()
    w.u(8, 77).u(8, 0).u(8, 40).ue(sps_id).ue(0).ue(2).ue(1).u(1, 0).ue(mb_w - 1).ue(mb_h - 1).u(1, 1).u(1, 1)
    if crop is None or not any(crop):
        w.u(1, 0)
    else:
        w.u(1, 1)
        for v in crop:
            w.ue(v)
    w.u(1, 0).trailing()
    return rbsp_to_nal(0x67, w.bytes())


def ipcm_pps(pps_id=0, sps_id=0):
    """CABAC, deblocking_filter_control_present_flag = 1, everything else at its simplest"""
    w = BitWriter()
    w.ue(pps_id).ue(sps_id).u(1, 1).u(1, 0).ue(0).ue(0).ue(0).u(1, 0).u(2, 0).se(0).se(0).se(0).u(1, 1).u(1, 0).u(1, 0)
    return rbsp_to_nal(0x68, w.trailing().bytes())


def ipcm_slice(mb_w, first_mb, count, planes, idr_pic_id=0, pps_id=0, slice_qp=26):
    """One IDR I slice of `count` I_PCM macroblocks from address first_mb.  planes = (Y, Cb, Cr): rows (bytes-like) of the coded
    picture, mb_w*16 luma and mb_w*8 chroma samples wide.  disable_deblocking_filter_idc = 1."""
    Y, Cb, Cr = planes
    w = BitWriter()
    w.ue(first_mb).ue(7).ue(pps_id).u(4, 0).ue(idr_pic_id)            # frame_num u(4): log2_max_frame_num_minus4 = 0; POC type 2
    w.u(1, 0).u(1, 0)                                                 # no_output_of_prior_pics, long_term_reference
    w.se(slice_qp - 26).ue(1)                                         # slice_qp_delta, disable_deblocking_filter_idc
    while not w.aligned():
        w.u(1, 1)                                                     # cabac_alignment_one_bit
    enc = CabacEncoder(w, slice_qp)
    for k in range(count):
        addr = first_mb + k
        mbx, mby = addr % mb_w, addr // mb_w
        # 9.3.3.1.1.3: ctxIdxInc of the first mb_type bin = the available neighbours A (left) and B (above) that are not I_NxN;
        # available means inside the picture and in this slice, and every macroblock here is I_PCM
        inc = int(mbx > 0 and addr - 1 >= first_mb) + int(mby > 0 and addr - mb_w >= first_mb)
        enc.decision(3 + inc, 1)                                      # mb_type != I_NxN
        enc.terminate(1)                                              # ... and it is I_PCM (Table 9-36: bins "1", terminate 1)
        while not w.aligned():
            w.u(1, 0)                                                 # pcm_alignment_zero_bit
        for r in range(16):                                           # 7.3.5: pcm_sample_luma[256], then pcm_sample_chroma[128]
            w.put_bytes(bytes(Y[mby * 16 + r][mbx * 16:mbx * 16 + 16]))
        for P in (Cb, Cr):
            for r in range(8):
                w.put_bytes(bytes(P[mby * 8 + r][mbx * 8:mbx * 8 + 8]))
        enc.init_engine()                                             # 9.3.1.2 after pcm samples; the contexts are kept
        enc.terminate(1 if k == count - 1 else 0)                     # end_of_slice_flag
    while not w.aligned():
        w.u(1, 0)                                                     # rbsp_alignment_zero_bit (the stop bit came from the flush)
    return rbsp_to_nal(0x65, w.bytes())


def ipcm_picture(mb_w, mb_h, planes, slice_per_row=False, idr_pic_id=0, pps_id=0):
    """the slice NAL units of one all-I_PCM IDR picture"""
    if slice_per_row:
        return [ipcm_slice(mb_w, r * mb_w, mb_w, planes, idr_pic_id, pps_id) for r in range(mb_h)]
    return [ipcm_slice(mb_w, 0, mb_w * mb_h, planes, idr_pic_id, pps_id)]
