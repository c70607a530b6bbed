"""Deterministic MPEG-TS inputs for the ingest-side (demux) parity tests: the synthetic muxer's plain video TS plus
hand-built variants that walk the branches of the reference demuxer (src/ts.js:43-148): other PIDs and stream ids,
PES_packet_length completion, PES headers without PTS, adaptation-field-only packets, stuffing inside a picture
(the frame-end guess fires early), a PID that changes its stream id, a garbage prefix (resync), a partial last packet."""
import functools

import numpy as np

from jsmpeg_amd import synth


def _pts_bytes(pts):
    return bytes([0x21 | ((pts >> 29) & 0x0e), (pts >> 22) & 0xff, 0x01 | ((pts >> 14) & 0xfe), (pts >> 7) & 0xff,
                  0x01 | ((pts << 1) & 0xfe)])


def pes_header(stream_id, payload_len_field=0, pts=None, extra_header=b""):
    flags = 0x80 if pts is not None else 0x00
    hdr = (_pts_bytes(pts) if pts is not None else b"") + extra_header
    plen = payload_len_field
    return bytes([0, 0, 1, stream_id, (plen >> 8) & 0xff, plen & 0xff, 0x80, flags, len(hdr)]) + hdr


class Muxer:
    def __init__(self):
        self.out = bytearray()
        self.cc = {}

    def packet(self, pid, payload=b"", pusi=False, stuffing=None, af_only=False):
        """One 188-byte packet.  stuffing: None = exactly as much as needed to fill; an int forces an adaptation field
        of that many bytes in total (>= 1).  Returns the number of payload bytes consumed."""
        cc = self.cc.get(pid, 0)
        self.cc[pid] = (cc + 1) & 15
        room = 184
        if af_only:
            pk = bytes([0x47, (0x40 if pusi else 0) | (pid >> 8), pid & 0xff, 0x20 | cc, 183, 0x00]) + b"\xff" * 182
            self.out += pk
            return 0
        need = stuffing if stuffing is not None else max(0, room - len(payload))
        take = min(len(payload), room - need)
        need = room - take
        pk = bytearray([0x47, (0x40 if pusi else 0) | (pid >> 8), pid & 0xff])
        if need:
            pk.append(0x30 | cc)
            pk.append(need - 1)
            if need > 1:
                pk.append(0x00)
                pk += b"\xff" * (need - 2)
        else:
            pk.append(0x10 | cc)
        pk += payload[:take]
        assert len(pk) == 188, len(pk)
        self.out += pk
        return take

    def pes(self, pid, stream_id, data, pts=None, with_length=False, split_first=True, mid_stuffing_at=None):
        """A PES packet over as many TS packets as it takes.  The last packet carries the stuffing (like the synthetic
        muxer); mid_stuffing_at = k puts 7 bytes of stuffing into packet k as well."""
        hdr_len_field = (3 + (5 if pts is not None else 0) + len(data)) if with_length else 0
        payload = pes_header(stream_id, hdr_len_field, pts) + bytes(data)
        k, first = 0, True
        while payload or first:
            if first and split_first and len(payload) <= 184 and len(payload) > 40:
                n = self.packet(pid, payload[:len(payload) // 2], pusi=True, stuffing=184 - len(payload) // 2)
            elif mid_stuffing_at is not None and k == mid_stuffing_at and len(payload) > 184:
                n = self.packet(pid, payload, pusi=first, stuffing=7)
            else:
                n = self.packet(pid, payload, pusi=first)
            payload = payload[n:]
            first = False
            k += 1

    def bytes(self):
        return np.frombuffer(bytes(self.out), dtype=np.uint8).copy()


def _pictures(n_frames=6, **ov):
    es, offs = synth.generate_config("cfg1_720p", n_frames=n_frames, width=176, height=144, **ov)
    pics = [bytes(es[int(offs[i]):int(offs[i + 1])]) for i in range(n_frames)]
    return es, pics


def _rng_bytes(seed, n):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def case_video_only():
    es, offs = synth.generate_config("cfg1_720p", n_frames=8, width=176, height=144)
    return synth.mux_ts(es, offs)


def case_video_audio_null():
    """Video PID 0x100 interleaved with an audio PES stream (0xC0, PES_packet_length set), null packets and a
    payload-start packet that is no PES (a PAT-like section)."""
    _, pics = _pictures(6)
    m = Muxer()
    for i, pic in enumerate(pics):
        m.packet(0x000, b"\x00\x00\xb0\x0d" + _rng_bytes(100 + i, 12), pusi=True)
        m.pes(0x100, 0xE0, pic, pts=9000 + 3000 * i)
        m.pes(0x101, 0xC0, _rng_bytes(i, 417), pts=9000 + 3000 * i, with_length=True)
        m.packet(0x1fff, b"\xff" * 184)
    return m.bytes()


def case_video_with_length_and_no_pts():
    """Video PES packets that carry PES_packet_length (completion by length, ts.js:134-146) -- the odd ones without
    a PTS (pts = 0, ts.js:97)."""
    _, pics = _pictures(6)
    m = Muxer()
    for i, pic in enumerate(pics):
        m.pes(0x100, 0xE0, pic, pts=None if i & 1 else 9000 + 3000 * i, with_length=True)
    return m.bytes()


def case_stuffing_inside_picture():
    """Stuffing in the middle of a picture: the frame-end guess (ts.js:143-146) completes the PES early, the rest
    arrives as a second write with the same pts.  Plus adaptation-field-only packets in between."""
    _, pics = _pictures(5, ac_max=12)
    m = Muxer()
    for i, pic in enumerate(pics):
        m.pes(0x100, 0xE0, pic, pts=9000 + 3000 * i, mid_stuffing_at=2)
        m.packet(0x100, af_only=True)
    return m.bytes()


def case_pid_changes_stream_id():
    """PID 0x100 starts as stream 0xE0, then carries a PES with stream id 0xE1 (its data must stop reaching the
    connected destination), then 0xE0 again."""
    _, pics = _pictures(6)
    m = Muxer()
    for i, pic in enumerate(pics):
        m.pes(0x100, 0xE1 if i in (2, 3) else 0xE0, pic, pts=9000 + 3000 * i)
    return m.bytes()


def case_garbage_prefix_resync():
    """50 bytes of garbage (without 0x47) before the first packet: ts.js resyncs (ts.js:150-187)."""
    ts = case_video_only()
    junk = np.frombuffer(bytes((b % 0x40) + 1 for b in _rng_bytes(7, 50)), dtype=np.uint8)
    return np.concatenate([junk, ts])


def case_partial_last_packet():
    ts = case_video_audio_null()
    return ts[:len(ts) - 100].copy()


def case_garbage_in_the_middle():
    """Junk between packets: 30 bytes without a sync byte after the tenth packet, later 200 bytes that contain lone 0x47
    bytes (false syncs: no four more behind them) -- ts.js drops the bad byte and resyncs each time (ts.js:43-50, 150-187)."""
    ts = case_video_audio_null()
    junk1 = np.frombuffer(bytes((b % 0x40) + 1 for b in _rng_bytes(11, 30)), dtype=np.uint8)
    j2 = bytearray((b % 0x40) + 0x80 for b in _rng_bytes(12, 200))
    j2[3] = 0x47; j2[60] = 0x47; j2[191] = 0x47
    junk2 = np.frombuffer(bytes(j2), dtype=np.uint8)
    return np.concatenate([ts[:188 * 10], junk1, ts[188 * 10:188 * 25], junk2, ts[188 * 25:]])


# ---------------------------------------------------------------------------------------------------------------------
# Scripted packets: a list of packet descriptions in, exactly ONE 188-byte packet per entry out, so that a case can say
# "packet 255 is X".  Payload bytes are seeded random: nothing of these cases is decoded as video.

def hdr(sid, length=0, pts=None, extra=b"", hlen=None):
    """A PES header: stream id, the PES_packet_length field as written, PTS or None, further header bytes; hlen
    overrides the PES_header_data_length byte (default: what is there)."""
    return dict(sid=sid, length=length, pts=pts, extra=bytes(extra), hlen=hlen)


def pkt(pid, pusi=False, af=None, af_len=None, pes=None, data=None):
    """One packet: PID, payload_unit_start, adaptation_field_control (default 1; 3 when af_len is given; 2 = adaptation
    field only, 0 = reserved), the adaptation_field_length byte (default 183 for af == 2), a PES header (hdr()) in front
    of the payload, and the first payload bytes (the rest of the packet is seeded random)."""
    if af is None:
        af = 1 if af_len is None else 3
    if (af & 2) and af_len is None:
        af_len = 183
    return dict(pid=pid, pusi=bool(pusi), af=af, af_len=af_len if af & 2 else None, pes=pes if af & 1 else None,
                data=bytes(data) if data is not None and af & 1 else None)


def _hdr_bytes(h):
    body = (_pts_bytes(h["pts"]) if h["pts"] is not None else b"") + h["extra"]
    hlen = len(body) if h["hlen"] is None else h["hlen"]
    ln = h["length"]
    return bytes([0, 0, 1, h["sid"], (ln >> 8) & 0xff, ln & 0xff, 0x80, 0x80 if h["pts"] is not None else 0x00, hlen]) + body


def hdr_len(h):
    """PES_header_data_length as written."""
    return h["hlen"] if h["hlen"] is not None else (5 if h["pts"] is not None else 0) + len(h["extra"])


def room(p):
    """Payload bytes the packet hands to its stream (ts.js:140-141: end - start); negative when a header runs past the
    packet, 0 for packets without payload."""
    if not p["af"] & 1:
        return 0
    at = 4 + ((1 + p["af_len"]) if p["af"] & 2 else 0)
    if p["pes"] is not None:
        at += 9 + hdr_len(p["pes"])
    return 188 - at


def set_length(script, at, complete_at):
    """Gives the PES header of script[at] the PES_packet_length that the payload of its PID's packets reaches exactly
    with packet complete_at."""
    h, pid = script[at]["pes"], script[at]["pid"]
    total = sum(room(p) for p in script[at:complete_at + 1] if p["pid"] == pid)
    assert script[complete_at]["pid"] == pid and room(script[complete_at]) > 0
    h["length"] = total + hdr_len(h) + 3
    assert 0 < h["length"] < 65536, h["length"]


def build(script, seed):
    rng = np.random.default_rng(seed)
    out, cc = bytearray(), {}
    for p in script:
        pid, af = p["pid"], p["af"]
        c = cc.get(pid, 0)
        if af & 1:
            cc[pid] = (c + 1) & 15
        pk = bytearray([0x47, (0x40 if p["pusi"] else 0) | (pid >> 8), pid & 0xff, (af << 4) | c])
        if af & 2:
            n = p["af_len"]
            pk.append(n)
            pk += (b"\x00" + b"\xff" * (n - 1))[:min(n, 188 - len(pk))]
        fill = rng.integers(0, 256, 184, dtype=np.uint8).tobytes()
        if af & 1 and len(pk) < 188:
            if p["pes"] is not None:
                pk += _hdr_bytes(p["pes"])[:188 - len(pk)]
            elif p["data"] is None and p["pusi"]:
                fill = bytes([fill[0] | 2]) + fill[1:]            # a payload start that is no PES does not begin 00 00 01
            if p["data"] is not None:
                assert len(pk) + len(p["data"]) <= 188
                pk += p["data"]
        elif af == 2:
            fill = b"\xff" * 184
        pk += fill[:188 - len(pk)]
        assert len(pk) == 188
        out += pk
    return np.frombuffer(bytes(out), dtype=np.uint8).copy()


V, V2, A = 0x100, 0x101, 0x102      # PIDs of the scripted cases


def _start(pid, sid, pts=None, length=0, **kw):
    return pkt(pid, pusi=True, pes=hdr(sid, length, pts), **kw)


def _video_pes(pid, sid, pts, n):
    """A PES without PES_packet_length over n packets; the last one is stuffed (the frame-end guess completes it)."""
    return [_start(pid, sid, pts)] + [pkt(pid) for _ in range(n - 2)] + [pkt(pid, af_len=20)]


def _filler(n, pid=V, sid=0xE0, pts0=90000):
    out = []
    while len(out) < n:
        out += _video_pes(pid, sid, pts0 + 3000 * len(out), min(5, n - len(out)) if n - len(out) != 6 else 3)
    assert len(out) == n and all(room(p) > 0 for p in out)
    return out


def script_chunk_carry_length(complete_at):
    """Video PES with PES_packet_length: the header is packet 250, the packet that completes it by length is
    `complete_at` -- lane 255 of the chunk of the header, lane 0 and lane 1 of the next.  After it the PID goes on
    without a header (nothing pending any more) until stuffing ends that."""
    s = _filler(250)
    s.append(_start(V, 0xE0, pts=777777, length=1))
    s += [pkt(V) for _ in range(complete_at - 250)]
    set_length(s, 250, complete_at)
    s += [pkt(V) for _ in range(9)] + [pkt(V, af_len=33)]
    s += _filler(300 - len(s))
    return s


def script_chunk_carry_length_far():
    """The header lies in chunk 0 (packet 100), the completing packet in chunk 2 (packet 620); every second packet in
    between is an audio PES of another PID that completes inside its own packet."""
    s = _filler(100)
    s.append(_start(V, 0xE0, pts=555555, length=1))
    for i in range(101, 621):
        if i % 2 == 0:
            s.append(pkt(V))
        else:
            s.append(_start(A, 0xC0, pts=3000 * i))
            s[-1]["pes"]["length"] = room(s[-1]) + 5 + 3
    set_length(s, 100, 620)
    s += [pkt(V) for _ in range(5)] + [pkt(V, af_len=7)]
    s += _filler(700 - len(s))
    return s


def script_chunk_carry_pid_map():
    """PID 0x100 changes from 0xE0 to 0xE1 by a header at packet 255 (the last lane of chunk 0) and back by a header at
    packet 512 (lane 0 of chunk 2); PID 0x101 carries 0xE0 all along, both feed the destination interleaved."""
    s = [_start(V2, 0xE0, pts=1000), _start(V, 0xE0, pts=2000)]
    for i in range(2, 620):
        sid = 0xE1 if 255 <= i < 512 else 0xE0
        if i == 255 or i == 512:
            s.append(_start(V, sid, pts=4000 + i))
        elif i % 16 == 0:
            s.append(_start(V2, 0xE0, pts=4000 + i))
        elif i % 16 == 8:
            s.append(_start(V, sid, pts=4000 + i))
        elif i % 5 == 4:
            s.append(pkt(V if i % 2 else V2, af_len=10))
        else:
            s.append(pkt(V if i % 2 else V2))
    return s


WAVE_EDGES = (0, 63, 64, 127, 128, 191, 192, 255)


def script_wave_edges():
    """Chunk 0: PES starts of the connected stream at lanes 0, 63, 64, 127, 128, 191, 192, 255, alternately with a
    PES_packet_length (of three packets) and without one.  Chunk 1: starts at lanes 63, 127, 191, 255 with that length
    (and one without at lane 0), so that each completes two lanes on, in the NEXT wave (the last in the next chunk).
    Every other packet continues the PID, a few of them stuffed.  Whether a continuation packet may complete by length
    depends on the last start at or before its lane."""
    s = []
    for i in range(512):
        c, lane = divmod(i, 256)
        if lane in (WAVE_EDGES if c == 0 else (0, 63, 127, 191, 255)):
            p = _start(V, 0xE0, pts=100000 + 3000 * i)
            if (WAVE_EDGES.index(lane) % 2 == 0) if c == 0 else lane != 0:
                p["pes"]["length"] = room(p) + 2 * 184 + 5 + 3
            s.append(p)
        elif lane in (30, 100, 160, 220):
            s.append(pkt(V, af_len=5))
        else:
            s.append(pkt(V))
    s += [pkt(V) for _ in range(5)] + [pkt(V, af_len=9)]
    return s


def script_two_headers_one_pid_one_chunk():
    """PID 0x100 gets 0xE0, 0xE1, 0xE0 headers within 40 packets of one chunk (50, 60, 70: the 0xE1 stretch crosses the
    wave edge at 64), and again across a chunk edge (250, 254, 258)."""
    s = []
    for i in range(300):
        if i in (0, 50, 70, 250, 258):
            s.append(_start(V, 0xE0, pts=9000 + i))
        elif i in (60, 254):
            s.append(_start(V, 0xE1, pts=9000 + i))
        elif i % 11 == 9:
            s.append(pkt(V, af_len=3))
        else:
            s.append(pkt(V))
    return s


def script_dense_writes(n, lead=0):
    """Alternately a PES start without PES_packet_length and without stuffing, and a PES start whose length is satisfied
    inside its own packet: the second yields TWO writes (the payload start completes the PES before it, its own data
    completes itself).  Every packet is a candidate of the walk; `lead` null packets in front are none."""
    s = [pkt(0x1fff) for _ in range(lead)]
    for i in range(n):
        p = _start(V, 0xE0, pts=200000 + 1500 * i)
        if i & 1:
            p["pes"]["length"] = room(p) + 5 + 3
        s.append(p)
    return s


PTS_33 = ((1 << 32) - 1, 1 << 32, (1 << 33) - 1, 0, 12345, None, (1 << 32) + 5, None)


def script_pts_33_bits():
    s = []
    for pts in PTS_33:
        s += [_start(V, 0xE0, pts), pkt(V), pkt(V, af_len=40)]
    return s


def script_negative_total():
    """PES_packet_length below header_length + 3: totalLength is negative, the PES completes with the first data --
    170 bytes of its own packet, none at all where the header fills the packet, or the packet after it."""
    s = _video_pes(V, 0xE0, 9000, 4)
    s.append(_start(V, 0xE0, pts=12000, length=1))                                   # 4: completes itself
    s += [pkt(V), pkt(V)]                                                            # 5, 6: no header pending
    s.append(pkt(V, pusi=True, pes=hdr(0xE0, 1, 15000, extra=b"\xff" * 170)))        # 7: 0 bytes of payload, a write of 0 bytes
    s += [pkt(V), pkt(V, af_len=12)]                                                 # 8, 9
    s.append(pkt(V, pusi=True, pes=hdr(0xE0, 2, None, extra=b"\xff" * 3)))           # 10: no PTS, total -4
    s += [pkt(V), pkt(V, af_len=1)]
    s += _filler(20 - len(s))
    return s


def script_reserved_and_af_only():
    """adaptation_field_control 0 (reserved) and 2 (no payload) on the connected PID, with and without
    payload_unit_start, and a payload start that is no PES while data is pending: with payload_unit_start each
    completes what is pending, none of them starts a PES (the pts of what follows stays)."""
    s = [_start(V, 0xE0, pts=30000), pkt(V), pkt(V)]
    s += [pkt(V, af=0), pkt(V)]                     # 3: nothing
    s += [pkt(V, af=0, pusi=True), pkt(V)]          # 5: completes
    s += [pkt(V, af=2), pkt(V)]                     # 7: nothing
    s += [pkt(V, af=2, pusi=True), pkt(V)]          # 9: completes
    s += [pkt(V, pusi=True), pkt(V)]                # 11: completes, and its payload is data
    s += [pkt(V, pusi=True, af_len=30), pkt(V, af_len=2)]
    s += [pkt(V, af=0, pusi=True), pkt(V, af=2, pusi=True)]     # nothing pending: no write
    s += _filler(24 - len(s))
    return s


def script_n_pids(n):
    """n PIDs with PES headers, even ones 0xE0 and odd ones 0xC0; 16 is the device's limit."""
    s = [_start(0x100 + k, 0xC0 if k & 1 else 0xE0, pts=9000 + k) for k in range(n)]
    for r in range(3):
        s += [pkt(0x100 + k, af_len=17 if r == 2 else None) for k in range(n)]
    s += [_start(0x100 + k, 0xE0 if k & 1 else 0xC0, pts=19000 + k) for k in range(n)]
    s += [pkt(0x100 + k, af_len=29) for k in range(n)]
    return s


END_AT = 8      # the packet of the end_of_data cases


def script_end_of_data(n=24):
    """Packet 8 is a payload start with nothing but an adaptation field of 183 bytes on the connected PID: what ts.js
    looks at for a start code are the bytes AFTER the packet.  At the end of the written data that counts as a start
    code with stream id 0 (the PID loses its stream id, packets 9-12 are dropped); anywhere else the next packet's sync
    byte is none."""
    s = _video_pes(V, 0xE0, 9000, 5) + [_start(V, 0xE0, 12000), pkt(V), pkt(V)]
    s.append(pkt(V, pusi=True, af=3, af_len=183))
    s += [pkt(V), pkt(V), pkt(V), pkt(V, af_len=50)]
    s += _filler(24 - len(s))
    return s[:n]


SPILL_AT = (6, 13, 17)      # the packets of the spill cases


def script_spill():
    """PES headers that begin so late in their packet that ts.js reads the stream id (packet 6), the length (13) or
    header_length (17) from the bytes after the packet.  Packet 6 ends 00 00 01: the stream id is the next byte."""
    s = _video_pes(V, 0xE0, 9000, 4) + [_start(V, 0xE0, 12000), pkt(V)]
    s.append(pkt(V, pusi=True, af_len=180, data=b"\x00\x00\x01"))
    s += [pkt(V), pkt(V), pkt(V)]
    s += [_start(V, 0xE0, 15000), pkt(V), pkt(V, af_len=4)]
    s.append(pkt(V, pusi=True, af_len=178, data=b"\x00\x00\x01\xe1\x00"))
    s += [pkt(V), _start(V, 0xE0, 18000), pkt(V, af_len=4)]
    s.append(pkt(V, pusi=True, af_len=175, data=b"\x00\x00\x01\xe1\x00\x00\x80\x80"))
    s += [pkt(V), _start(V, 0xE0, 21000), pkt(V), pkt(V, af_len=4)]
    s += _filler(32 - len(s))
    return s


def case_spill_junk():
    """The same with 30 bytes of junk after packet 6: ts.js takes the stream id (0xE0), length, flags and
    header_length from the junk and resyncs behind it."""
    ts = build(script_spill(), 113)
    junk = bytearray((b % 0x40) + 1 for b in _rng_bytes(13, 30))
    junk[:6] = bytes([0xE0, 0x00, 0x00, 0x80, 0x00, 0x00])
    at = 188 * (SPILL_AT[0] + 1)
    return np.concatenate([ts[:at], np.frombuffer(bytes(junk), dtype=np.uint8), ts[at:]])


def script_header_past_packet():
    """Packet 2: a PES header of the connected stream whose header_length puts the payload behind the packet."""
    s = [_start(V, 0xE0, 9000), pkt(V)]
    s.append(pkt(V, pusi=True, pes=hdr(0xE0, 0, 12000, hlen=200)))
    s += [pkt(V), pkt(V, af_len=8)]
    s += _filler(12 - len(s))
    return s


SCRIPTS = {
    "chunk_carry_length_255": (lambda: script_chunk_carry_length(255), 101),
    "chunk_carry_length_256": (lambda: script_chunk_carry_length(256), 102),
    "chunk_carry_length_257": (lambda: script_chunk_carry_length(257), 103),
    "chunk_carry_length_far": (script_chunk_carry_length_far, 104),
    "chunk_carry_pid_map": (script_chunk_carry_pid_map, 105),
    "wave_edges": (script_wave_edges, 106),
    "two_headers_one_pid_one_chunk": (script_two_headers_one_pid_one_chunk, 107),
    "dense_writes": (lambda: script_dense_writes(600), 108),
    "pts_33_bits": (script_pts_33_bits, 109),
    "negative_total": (script_negative_total, 110),
    "reserved_and_af_only": (script_reserved_and_af_only, 111),
    "sixteen_pids": (lambda: script_n_pids(16), 112),
    "seventeen_pids": (lambda: script_n_pids(17), 112),
    "spill_adjacent": (script_spill, 113),
    "header_past_packet": (script_header_past_packet, 114),
    "end_of_data_inner_write": (script_end_of_data, 115),
    "end_of_data_inner_partial": (script_end_of_data, 115),
    "end_of_data_last": (lambda: script_end_of_data(END_AT + 1), 115),
}
DENSE_COUNTS = (0, 1, 7, 8, 9, 16)      # candidates of the walk: none, one, either side of its groups of eight
for _n in DENSE_COUNTS:
    SCRIPTS["dense_writes_%d" % _n] = (lambda _n=_n: script_dense_writes(_n, lead=3), 108)


def scripted(name):
    fn, seed = SCRIPTS[name]
    return build(fn(), seed)


def case_end_of_data_before_partial():
    """... as the last whole packet in front of a partial one: ts.js reads on into the partial packet (a sync byte: no
    start code), for the device the data ends with the last whole packet."""
    ts = build(script_end_of_data(), 115)
    return ts[:188 * (END_AT + 1) + 60].copy()


CASES = {
    "video_only": case_video_only,
    "video_audio_null": case_video_audio_null,
    "video_with_length_and_no_pts": case_video_with_length_and_no_pts,
    "stuffing_inside_picture": case_stuffing_inside_picture,
    "pid_changes_stream_id": case_pid_changes_stream_id,
    "garbage_prefix_resync": case_garbage_prefix_resync,
    "partial_last_packet": case_partial_last_packet,
    "garbage_in_the_middle": case_garbage_in_the_middle,
    "spill_junk": case_spill_junk,
    "end_of_data_before_partial": case_end_of_data_before_partial,
}
for _name in SCRIPTS:
    CASES[_name] = (lambda _name=_name: scripted(_name))

# the same buffers handed to the demuxer in SEVERAL write() calls (ts.js:25-41: leftover bytes); the last size takes the rest
WRITES = {
    "video_only": [1000, 333, 188 * 5 + 7, 1, 187, 1 << 30],
    "garbage_prefix_resync": [40, 100, 1200, 188, 1 << 30],          # the first resync attempts run out of data
    "garbage_in_the_middle": [188 * 10 + 5, 600, 188 * 14, 150, 300, 2000, 1 << 30],
    "partial_last_packet": [5000, 5000, 1 << 30],
    "end_of_data_inner_write": [188 * (END_AT + 1), 1 << 30],          # packet 8 ends the first write()
    "end_of_data_inner_partial": [188 * (END_AT + 1) + 50, 1 << 30],   # ... 50 bytes of packet 9 behind it
}

# What the device demux refuses (upload_ts raises with this in its message) instead of matching ts.js; the key is the
# fixture: the case, and whether it is the one of its WRITES.  These fixtures are tests/golden/excluded_ts_*.json.
REFUSED = {
    ("seventeen_pids", False): "more than 16 PIDs",
    ("header_past_packet", False): "runs past the end of its TS packet",
    ("spill_junk", False): "reads past the packet's end",
    ("end_of_data_inner_write", True): "reads past the packet's end",
    ("end_of_data_before_partial", False): "reads past the packet's end",
}


# ---------------------------------------------------------------------------------------------------------------------
# The random sweep of the device demux (tests/test_gpu_ts_walk.py) and of the host demuxer; its conditions are checked
# on the restatement alone (tests/test_ts_walk_cases.py).

SWEEP_SIDS = (0xE0, 0xE1, 0xC0)
SWEEP_BATCHES = 30
SWEEP_FIXED = (0, 1, 255, 256, 257)     # one stream of every batch has this many packets


def random_script(rng, n):
    """n packets: 2 to 6 PIDs with stream ids of SWEEP_SIDS (now and then a PID changes its id); PES packets of 1 to 6
    packets with or without PES_packet_length (reached exactly with the last packet, earlier, or never), with or
    without PTS (33 bits), stuffing in the middle and at the end; null packets, adaptation-field-only and reserved
    packets, payload starts that are no PES.  No header reaches past its packet."""
    n_pids = int(rng.integers(2, 7))
    pids = [0x100 + 3 * k for k in range(n_pids)]
    sid = {p: SWEEP_SIDS[int(rng.integers(0, 3))] for p in pids}
    sid[pids[0]], sid[pids[1]] = 0xE0, 0xC0
    queue = {p: [] for p in pids}

    def plan(pid):
        if rng.random() < 0.1:
            sid[pid] = SWEEP_SIDS[int(rng.integers(0, 3))]
        h = hdr(sid[pid], 0, int(rng.integers(0, 1 << 33)) if rng.random() < 0.7 else None,
                extra=b"\xff" * int(rng.integers(1, 4)) if rng.random() < 0.2 else b"")
        ps = [pkt(pid, pusi=True, pes=h, af_len=int(rng.integers(0, 40)) if rng.random() < 0.15 else None)]
        k = int(rng.integers(1, 7))
        for j in range(1, k):
            stuffed = rng.random() < (0.6 if j == k - 1 else 0.1)
            ps.append(pkt(pid, af_len=int(rng.integers(0, 100)) if stuffed else None))
        if rng.random() < 0.45:
            total, mode = sum(room(p) for p in ps), rng.random()
            want = total if mode < 0.6 else max(1, total - int(rng.integers(1, 200))) if mode < 0.8 else total + int(rng.integers(1, 400))
            h["length"] = want + hdr_len(h) + 3
        return ps

    out = []
    while len(out) < n:
        r, pid = rng.random(), pids[int(rng.integers(0, n_pids))]
        if r < 0.05:
            out.append(pkt(0x1fff))
        elif r < 0.08:
            out.append(pkt(pid, af=2, pusi=rng.random() < 0.3))
        elif r < 0.10:
            out.append(pkt(pid, af=0, pusi=rng.random() < 0.3))
        elif r < 0.13:
            out.append(pkt(pid, pusi=True, af_len=int(rng.integers(0, 100)) if rng.random() < 0.3 else None))
        else:
            if not queue[pid]:
                queue[pid] = plan(pid)
            out.append(queue[pid].pop(0))
    return out


def sweep_batch(b):
    """The 8 streams of batch b: packet counts on both sides of 256 and of 512, one of SWEEP_FIXED."""
    rng = np.random.default_rng(1000 + b)
    counts = [SWEEP_FIXED[b % 5], int(rng.integers(2, 255)), int(rng.integers(258, 512)),
              513 if b % 4 == 0 else int(rng.integers(514, 640))] + [int(x) for x in rng.integers(2, 640, 4)]
    return [build(random_script(rng, n), int(rng.integers(0, 1 << 31))) for n in counts]


def _pieces(rng, n):
    sizes = []
    while n > 0:
        sizes.append(int(min(n, rng.randint(1, 4000))))
        n -= sizes[-1]
    return sizes


@functools.lru_cache(maxsize=None)
def sweep_runs(b):
    """Batch b three ways, as (way, streams, write sizes or None): in one write() each; in write() calls of random
    sizes; with junk spliced between packets and a truncated end (the recipe of the packet framing test: every third
    batch's junk without sync bytes, three batches of four in write() calls of random sizes)."""
    base = sweep_batch(b)
    rng = np.random.RandomState(2000 + b)
    runs = [("one_write", base, None), ("pieces", base, [_pieces(rng, len(ts)) for ts in base])]
    damaged = []
    for ts in base:
        parts, at, n_pk = [], 0, len(ts) // 188
        cuts = sorted(rng.choice(np.arange(1, n_pk), size=rng.randint(0, 4), replace=False)) if n_pk > 4 else []
        for cut in cuts:
            parts.append(ts[at:cut * 188])
            junk = rng.randint(0, 256, size=rng.randint(1, 1300)).astype(np.uint8)
            if b % 3 == 0:
                junk[junk == 0x47] = 0x48
            parts.append(junk)
            at = cut * 188
        parts.append(ts[at:max(at, len(ts) - rng.randint(0, 400))])
        damaged.append(np.ascontiguousarray(np.concatenate(parts)))
    runs.append(("damaged", damaged, [_pieces(rng, len(ts)) for ts in damaged] if b % 4 else None))
    return runs


def sweep_stream_id(b):
    return 0xC0 if b % 3 == 1 else 0xE0
