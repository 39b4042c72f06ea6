"""A restatement, on decoder states only, of stages 1-2 of the device JPEG decoder (i-vit_amd/csrc/jpeg.hip: sync_kernel and
fix_kernel).  Plain Python / numpy: it parses DHT, SOF, DRI and SOS itself, de-stuffs the scan, and steps codewords as huff_step
does -- state (bit position in the restart segment, block of the MCU, coefficient index), a 16-bit advance with symbol 0 on a code
no table holds.  It writes no coefficients and is no oracle for pixels: it says which path an input takes (how many neighbour
rounds a lane needs, how far the serial continuation runs at a 256-lane boundary), so that "this batch exercises that path" is an
assertion, and it shows on the CPU that an input depends on a stage (after_sync != true where the continuation has work to do).

    segments(data)                      de-stuffed bytes per restart segment
    subsequences(data)                  subsequences per restart segment, ceil(8 n / 4096), 1 for an empty segment
    decoded_blocks(data)                per segment: (blocks decoded from the true state, the MCUs' blocks, bits left over)
    sync_states(data, first_global_sub) the states of every subsequence through sync_kernel and fix_kernel
"""
from dataclasses import dataclass, field

import numpy as np

SUB_BITS = 4096
LANES = 256


@dataclass
class Frame:
    h: int = 0
    w: int = 0
    ncomp: int = 0
    restart: int = 0
    bpm: int = 0
    mcux: int = 0
    mcuy: int = 0
    blk_dc: list = field(default_factory=list)      # block of the MCU -> 16-bit lookup of its DC table
    blk_ac: list = field(default_factory=list)
    segs: list = field(default_factory=list)        # de-stuffed bytes per restart segment

    @property
    def nmcu(self):
        return self.mcux * self.mcuy

    def seg_mcus(self, i):
        per = self.restart or self.nmcu
        return min(per, self.nmcu - i * per)


def _lookup(bits, vals):
    """16-bit window -> (length << 8) | symbol; 0 where no code of the table matches (lengths are >= 1, so 0 is free)"""
    lut = np.zeros(1 << 16, np.int32)
    code, k = 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            lo = code << (16 - length)
            lut[lo:lo + (1 << (16 - length))] = (length << 8) | vals[k]
            code += 1
            k += 1
        code <<= 1
    return lut.tolist()


def parse(data) -> Frame:
    d = bytes(data)
    assert d[:2] == b"\xff\xd8"
    F = Frame()
    tabs, comps, pos = {}, [], 2
    while True:
        assert d[pos] == 0xFF
        while d[pos] == 0xFF:
            pos += 1
        m = d[pos]
        pos += 1
        n = int.from_bytes(d[pos:pos + 2], "big")
        s = d[pos + 2:pos + n]
        pos += n
        if m in (0xC0, 0xC1):
            F.h, F.w, F.ncomp = int.from_bytes(s[1:3], "big"), int.from_bytes(s[3:5], "big"), s[5]
            comps = [(s[6 + 3 * c], s[7 + 3 * c] >> 4, s[7 + 3 * c] & 15) for c in range(F.ncomp)]
        elif m == 0xC4:
            k = 0
            while k < len(s):
                bits = list(s[k + 1:k + 17])
                cnt = sum(bits)
                tabs[s[k]] = _lookup(bits, list(s[k + 17:k + 17 + cnt]))      # key: (class << 4) | id
                k += 17 + cnt
        elif m == 0xDD:
            F.restart = int.from_bytes(s[:2], "big")
        elif m == 0xDA:
            assert s[0] == F.ncomp
            sel = [(s[2 + 2 * c] >> 4, s[2 + 2 * c] & 15) for c in range(F.ncomp)]
            break
    if F.ncomp == 1:            # a non-interleaved scan: one block per MCU
        hmax = vmax = 1
        per = [1]
    else:
        hmax, vmax = comps[0][1], comps[0][2]
        per = [h * v for _, h, v in comps]
    F.bpm = sum(per)
    F.mcux = (F.w + 8 * hmax - 1) // (8 * hmax)
    F.mcuy = (F.h + 8 * vmax - 1) // (8 * vmax)
    for c, nb in enumerate(per):
        F.blk_dc += [tabs[sel[c][0]]] * nb
        F.blk_ac += [tabs[0x10 | sel[c][1]]] * nb
    # the scan: 0xFF 0x00 -> 0xFF, fill 0xFF bytes skipped, RSTn closes a segment, any other marker ends it
    seg = bytearray()
    n = len(d)
    while pos < n:
        nxt = d.find(b"\xff", pos)
        if nxt < 0:
            break
        seg += d[pos:nxt]
        pos = nxt + 1
        while pos < n and d[pos] == 0xFF:
            pos += 1
        if pos >= n:
            break
        m = d[pos]
        pos += 1
        if m == 0:
            seg.append(0xFF)
        elif 0xD0 <= m <= 0xD7:
            F.segs.append(bytes(seg))
            seg = bytearray()
        else:
            break
    F.segs.append(bytes(seg))
    return F


def segments(data):
    """de-stuffed byte length of every restart segment"""
    return [len(s) for s in parse(data).segs]


def _nsub(nbytes):
    return max((8 * nbytes + SUB_BITS - 1) // SUB_BITS, 1)


def subsequences(data):
    return [_nsub(n) for n in segments(data)]


class _Seg:
    """one restart segment: run(state, end) decodes the codewords that start before bit `end` (run_sub)"""

    def __init__(self, F, raw):
        self.F, self.n, self.d = F, len(raw), raw + bytes(8)      # bytes past the segment read as 0
        self.memo = {}

    def run(self, state, end, limit=None):
        key = (state, end)
        if limit is None and key in self.memo:
            return self.memo[key]
        p, blk, z = state
        d, dc, ac, bpm = self.d, self.F.blk_dc, self.F.blk_ac, self.F.bpm
        count = 0
        while p < end and (limit is None or count < limit):
            w = (int.from_bytes(d[p >> 3:(p >> 3) + 5], "big") >> (8 - (p & 7))) & 0xFFFFFFFF
            e = (dc[blk] if z == 0 else ac[blk])[w >> 16]
            if e:
                length, sym = e >> 8, e & 255
            else:
                length, sym = 16, 0
            size = sym if z == 0 else sym & 15
            p += length + size
            if z == 0:
                z = 1
            elif size:
                z += (sym >> 4) + 1
            elif sym >> 4 == 15:
                z += 16
            else:
                z = 64
            if z >= 64:
                z = 0
                blk = 0 if blk + 1 == bpm else blk + 1
                count += 1
        out = ((p, blk, z), count)
        if limit is None:
            self.memo[key] = out
        return out


def decoded_blocks(data):
    """per restart segment: (blocks decoded serially from the segment's start, stopping at its MCUs' blocks as the decoders do;
    the blocks its MCUs hold; the bits left over, which in a sound file are fewer than 8 padding bits)"""
    F = parse(data)
    out = []
    for i, raw in enumerate(F.segs):
        want = F.seg_mcus(i) * F.bpm
        (p, _, _), count = _Seg(F, raw).run((0, 0, 0), 8 * len(raw), limit=want)
        out.append((count, want, 8 * len(raw) - p))
    return out


@dataclass
class SyncStates:
    seg_of: list          # per subsequence of the image: its restart segment
    true_in: list         # the true entry state (p, blk, z): serial decoding from the segment's start
    guess_out: list       # the exit state when decoded from the guessed state (start bit, block 0, coefficient 0)
    rounds: list          # the last neighbour round of sync_kernel in which the lane took a new entry state (0: none)
    after_sync_in: list   # st_in after sync_kernel
    after_sync_out: list
    final_in: list        # st_in after fix_kernel
    final_out: list
    final_cnt: list       # blocks completed per subsequence, after fix_kernel
    boundaries: list      # (local subsequence on a 256-multiple of the global index, "first" if it starts a segment,
    #                        else the number of subsequences the continuation re-decoded), boundaries it ran through not listed


def sync_states(data, first_global_sub, continuation=True) -> SyncStates:
    """sync_kernel and fix_kernel on one image whose first subsequence has the global index first_global_sub.  With
    continuation=False fix_kernel is left out (final_* = after_sync_*)."""
    F = parse(data)
    segs = [_Seg(F, raw) for raw in F.segs]
    seg_of, k_in, seg_first = [], [], []
    for i, s in enumerate(segs):
        seg_first.append(len(seg_of))
        for k in range(_nsub(s.n)):
            seg_of.append(i)
            k_in.append(k)
    nsub = len(seg_of)
    bits = [8 * s.n for s in segs]
    start = [k * SUB_BITS for k in k_in]
    end = [min(start[j] + SUB_BITS, bits[seg_of[j]]) for j in range(nsub)]

    true_in, st = [], None
    for j in range(nsub):
        if k_in[j] == 0:
            st = (0, 0, 0)
        true_in.append(st)
        st, _ = segs[seg_of[j]].run(st, end[j])

    entry = [(start[j], 0, 0) for j in range(nsub)]
    res = [segs[seg_of[j]].run(entry[j], end[j]) for j in range(nsub)]
    exit_, cnt = [r[0] for r in res], [r[1] for r in res]
    guess_out = list(exit_)
    rounds = [0] * nsub
    g0 = first_global_sub
    lo = 0
    while lo < nsub:       # one 256-lane workgroup at a time: the lanes of this image in it
        hi = min(nsub, lo + LANES - (g0 + lo) % LANES)
        for rnd in range(1, LANES + 1):
            changed = []
            for j in range(lo + 1, hi):       # lane lo is the workgroup's lane 0 or a segment's first subsequence
                if k_in[j] and seg_of[j - 1] == seg_of[j] and exit_[j - 1] != entry[j]:
                    changed.append((j, exit_[j - 1]))
            if not changed:
                break
            for j, e in changed:              # all lanes read, then all write
                entry[j] = e
                (exit_[j], cnt[j]) = segs[seg_of[j]].run(e, end[j])
                rounds[j] = rnd
        lo = hi
    after_in, after_out = list(entry), list(exit_)

    boundaries = []
    if continuation:
        gb = (g0 + LANES) // LANES * LANES
        while gb < g0 + nsub:
            local = gb - g0
            si = seg_of[local]
            if local == seg_first[si]:
                boundaries.append((local, "first"))
                gb += LANES
                continue
            seg_end = seg_first[si] + _nsub(segs[si].n)
            redone = 0
            while local < seg_end:
                e = exit_[local - 1]
                if e == entry[local]:
                    break
                entry[local] = e
                x, cnt[local] = segs[si].run(e, end[local])
                redone += 1
                old, exit_[local] = exit_[local], x
                if x == old:
                    break
                local += 1
            boundaries.append((gb - g0, redone))
            if gb < g0 + local:
                gb = (g0 + local) // LANES * LANES
            gb += LANES
    return SyncStates(seg_of, true_in, guess_out, rounds, after_in, after_out, list(entry), list(exit_), list(cnt), boundaries)
