"""Guarded arenas for the C-ABI's memory contract (include/dmpc.h: "the caller owns every buffer; the library allocates
nothing, inputs are read-only", and every `*_workspace_bytes` query is enough).

One `torch.uint8` allocation holds every array of a call - inputs, outputs, `info`, workspace - each cut out as
`arena[off:off+n].view(dtype).view(shape)`, 16-byte aligned, with guard bands before, between and after them.  A band
(and the pad up to the next 16-byte boundary) holds the int32 word GUARD = 0x7FC5A5A5: a quiet NaN with a payload as float32
and, doubled, the float64 3.04e307 (no NaN: its exponent field is 0x7FC) - either way a value no result holds by chance.

    layout "A": 256-byte bands, arrays in declaration order; `out` and `ws` arrays prefilled with GUARD
    layout "B": 272-byte bands, the first array at offset 16, arrays in reverse order (base pointers 16 modulo 256, all the
                ABI asks for); `out` and `ws` arrays prefilled with the bits of 12345678.0f

Roles:  in     read-only; bit-equal after the call
        out    every word written (outside `unwritten`), bit-equal between the layouts (or within `tol`)
        inout  read and written; `unwritten` parts bit-equal after the call, the whole compared between the layouts
        ws     workspace of exactly the queried size; anything may be in it afterwards
        info   int32 flags: zeroed ("or": the call ORs into it) or prefilled ("written": the call writes it)
        pre    belongs to a preparing call only (its outputs that the checked call does not see); not examined

    b = Builder(); x = b.inp("x", array); y = b.out("y", (3, 4)); w = b.ws("ws", nbytes)
    a = b.build("A", device); ...the call, with a.ptr(x) ...; findings = a.check(rc)
    findings += a.compare(b_arena)       # layout A against layout B

Everything is examined on the host from ONE copy of the arena taken after the call (and one before it)."""
import struct

import numpy as np
import torch

GUARD = 0x7FC5A5A5
FILL_B = struct.unpack("<i", struct.pack("<f", 12345678.0))[0]
BAND = {"A": 256, "B": 272}
ROLES = ("in", "out", "inout", "ws", "info", "pre")

_NP = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64, np.dtype(np.int32): torch.int32,
       np.dtype(np.uint8): torch.uint8}


class Spec:
    """one array of a call: a handle before the arena exists, resolved by Arena.ptr / Arena.view afterwards"""

    def __init__(self, name, role, dtype, shape, init=None, unwritten=None, info_mode="or", tol=None, prefill=False):
        assert role in ROLES, role
        self.name, self.role, self.dtype, self.shape = name, role, np.dtype(dtype), tuple(int(s) for s in shape)
        assert self.dtype in _NP, dtype
        self.init = None if init is None else np.ascontiguousarray(np.asarray(init, dtype=self.dtype).reshape(self.shape))
        self.unwritten = None if unwritten is None else np.broadcast_to(np.asarray(unwritten, dtype=bool), self.shape).copy()
        self.info_mode, self.tol, self.prefill = info_mode, tol, prefill
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize

    def __repr__(self):
        return "<%s %s %s%s>" % (self.role, self.name, self.dtype, list(self.shape))


class Builder:
    """collects the arrays of one call in declaration order"""

    def __init__(self):
        self.specs = []

    def _add(self, spec):
        assert all(s.name != spec.name for s in self.specs), spec.name
        self.specs.append(spec)
        return spec

    def inp(self, name, array, dtype=np.float32):
        """an input with its values"""
        array = np.asarray(array)
        return self._add(Spec(name, "in", dtype, array.shape, init=array))

    def out(self, name, shape, dtype=np.float32, unwritten=None, tol=None):
        return self._add(Spec(name, "out", dtype, shape, unwritten=unwritten, tol=tol))

    def inout(self, name, array, dtype=np.float32, unwritten=None):
        array = np.asarray(array)
        return self._add(Spec(name, "inout", dtype, array.shape, init=array, unwritten=unwritten))

    def ws(self, name, nbytes):
        return self._add(Spec(name, "ws", np.uint8, (int(nbytes),)))

    def info(self, name, n, written=False):
        return self._add(Spec(name, "info", np.int32, (n,), info_mode="written" if written else "or"))

    def produced(self, name, shape, dtype=np.float32):
        """an input of the checked call that a preparing call writes (prefilled like an output until then)"""
        return self._add(Spec(name, "in", dtype, shape, prefill=True))

    def pre(self, name, shape, dtype=np.float32):
        return self._add(Spec(name, "pre", dtype, shape))

    def build(self, layout, device):
        return Arena(self.specs, layout, device)


def _round16(n):
    return (n + 15) // 16 * 16


class Arena:
    def __init__(self, specs, layout, device="cpu"):
        assert layout in BAND, layout
        self.layout, self.specs = layout, list(specs)
        band = BAND[layout]
        order = self.specs if layout == "A" else self.specs[::-1]
        off = band if layout == "A" else 16
        self.offset = {}
        for s in order:
            assert off % 16 == 0
            self.offset[s.name] = off
            off = _round16(off + s.nbytes) + band
        self.nbytes = off
        self.by_name = {s.name: s for s in self.specs}
        self.buf = torch.empty(self.nbytes, dtype=torch.uint8, device=device)
        assert self.buf.data_ptr() % 16 == 0
        self.buf.view(torch.int32).fill_(GUARD)
        fill = GUARD if layout == "A" else FILL_B
        for s in self.specs:
            if s.nbytes == 0:
                continue
            if s.init is not None:
                self.view(s).copy_(torch.from_numpy(s.init))
            elif s.role == "info" and s.info_mode == "or":
                self.view(s).zero_()
            elif s.role in ("out", "ws", "pre", "info") or s.prefill:
                self._fill(s, fill)
            else:
                self.view(s).zero_()
        self.guard_mask = np.ones(self.nbytes, dtype=bool)
        for s in self.specs:
            self.guard_mask[self.offset[s.name]:self.offset[s.name] + s.nbytes] = False
        self.guard_image = np.frombuffer(struct.pack("<i", GUARD) * (self.nbytes // 4), dtype=np.uint8)
        self.before = None
        self.after = None
        self.rc = None

    def _fill(self, s, word):
        """the int32 word over the array's bytes (a byte count that is no multiple of 4: the word's leading bytes)"""
        o, n = self.offset[s.name], s.nbytes
        self.buf[o:o + n // 4 * 4].view(torch.int32).fill_(word)
        if n % 4:
            tail = torch.from_numpy(np.frombuffer(struct.pack("<i", word), dtype=np.uint8)[:n % 4].copy())
            self.buf[o + n // 4 * 4:o + n].copy_(tail)

    def view(self, s):
        s = self.by_name[s] if isinstance(s, str) else s
        o = self.offset[s.name]
        return self.buf[o:o + s.nbytes].view(_NP[s.dtype]).view(s.shape)

    def ptr(self, s):
        """the array's device pointer (None -> NULL)"""
        if s is None:
            return None
        s = self.by_name[s] if isinstance(s, str) else s
        p = self.buf.data_ptr() + self.offset[s.name]
        assert p % 16 == 0
        return p

    def _image(self):
        return self.buf.cpu().numpy().copy()

    def snapshot(self):
        """the arena as the checked call finds it (after the preparing calls, synchronised by the caller)"""
        self.before = self._image()

    def host(self, s, image=None):
        """the array's values in an image of the arena (default: after the call)"""
        s = self.by_name[s] if isinstance(s, str) else s
        image = self.after if image is None else image
        o = self.offset[s.name]
        return image[o:o + s.nbytes].view(s.dtype).reshape(s.shape)

    def _bytes(self, s, image):
        o = self.offset[s.name]
        return image[o:o + s.nbytes]

    @staticmethod
    def _first(bad):
        return int(np.flatnonzero(bad)[0])

    def check(self, rc=0):
        """after the call and one synchronize(): -> list of findings, each naming the array and the first offending byte"""
        assert self.before is not None, "snapshot() before the call"
        self.after = self._image()
        self.rc = rc
        out = []
        # (a) guard words
        bad = self.guard_mask & (self.after != self.guard_image)
        if bad.any():
            at = self._first(bad)
            out.append("guard: byte %d of the arena overwritten (%s)" % (at, self._where(at)))
        for s in self.specs:
            if s.nbytes == 0:
                continue
            now, was = self._bytes(s, self.after), self._bytes(s, self.before)
            if rc < 0:
                # a refused call launched nothing
                if s.role != "pre" and (now != was).any():
                    out.append("%s: refused call (rc %d) wrote byte %d" % (s.name, rc, self._first(now != was)))
                continue
            if s.role == "in":
                # (b) inputs are read-only
                if (now != was).any():
                    out.append("%s: input modified at byte %d" % (s.name, self._first(now != was)))
                continue
            un = None
            if s.unwritten is not None:
                un = np.repeat(s.unwritten.reshape(-1), s.dtype.itemsize)
                if (un & (now != was)).any():
                    out.append("%s: region declared unwritten changed at byte %d" % (s.name, self._first(un & (now != was))))
            written = s.role == "out" or (s.role == "info" and s.info_mode == "written")
            if written and self.layout == "A" and s.nbytes % 4 == 0:
                # (c) no word still holds the guard
                left = np.repeat(now.view(np.int32) == GUARD, 4)
                if un is not None:
                    left &= ~un
                if left.any():
                    out.append("%s: not written at byte %d (%d words left)" % (s.name, self._first(left), int(left.sum()) // 4))
        return out

    def _where(self, at):
        """the array nearest to a byte of a guard band"""
        best = None
        for s in self.specs:
            o = self.offset[s.name]
            d, side = (o - at, "before") if at < o else (at - (o + s.nbytes) + 1, "past the end of")
            if best is None or d < best[0]:
                best = (d, "%d bytes %s %s" % (d, side, s.name))
        return best[1]

    def compare(self, other):
        """(d) the same call in the other layout: outputs bit-equal (within `tol`, relative to max(1, |ref|), where the
        array is declared with one: sums formed with float atomics)"""
        assert self.after is not None and other.after is not None
        if self.rc != other.rc:
            return ["return codes differ between the layouts: %d against %d" % (self.rc, other.rc)]
        if self.rc < 0:
            return []           # (nothing launched: every array still holds its layout's prefill, which check() has seen)
        out = []
        for s in self.specs:
            if s.role not in ("out", "inout", "info") or s.nbytes == 0:
                continue
            mine, theirs = self.host(s), other.host(other.by_name[s.name])
            keep = np.ones(s.shape, dtype=bool) if s.unwritten is None or s.role == "inout" else ~s.unwritten
            if s.tol is not None:
                err = np.abs(mine.astype(np.float64) - theirs) / np.maximum(1.0, np.abs(theirs.astype(np.float64)))
                bad = keep & ~(err <= s.tol)
            else:
                size = s.dtype.itemsize
                diff = (mine.reshape(-1).view(np.uint8) != theirs.reshape(-1).view(np.uint8)).reshape(-1, size).any(axis=1)
                bad = keep & diff.reshape(s.shape)
            if bad.any():
                at = self._first(bad.reshape(-1))
                out.append("%s: layouts differ at element %d (byte %d): %r against %r" % (
                    s.name, at, at * s.dtype.itemsize, mine.reshape(-1)[at], theirs.reshape(-1)[at]))
        return out
