"""Plain gzip variants of the FASTA edge text and of the tilapia contig (made
with Python's zlib only, written once per session): what tests/test_gzip_host.py
and tests/test_gzip_device.py read."""
import os
import struct
import zlib

from _util import TILAPIA_FA
from test_fasta_device import edge_text

_cache = {}

EDGE_VARIANTS = ("l6", "l1", "stored", "fixed", "mem1", "three")
ALL_VARIANTS = EDGE_VARIANTS + ("tilapia",)


def gz(data, level=6, mem=8, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, 31, mem, strategy)
    return c.compress(data) + c.flush()


def _member(data, flags, mem=1):
    """One gzip member with header fields: FEXTRA 4, FNAME 8, FCOMMENT 16, FHCRC 2."""
    h = bytearray(b"\x1f\x8b\x08" + bytes([flags]) + b"\0\0\0\0\0\x03")
    if flags & 4:
        h += struct.pack("<H", 6) + b"AB\x02\x00\x07\x09"
    if flags & 8:
        h += b"edge part.fa\0"
    if flags & 16:
        h += b"a comment, with a \x1f\x8b in it\0"
    if flags & 2:
        h += struct.pack("<H", zlib.crc32(bytes(h)) & 0xffff)
    c = zlib.compressobj(6, zlib.DEFLATED, -15, mem)
    body = c.compress(data) + c.flush()
    return bytes(h) + body + struct.pack("<II", zlib.crc32(data), len(data) & 0xffffffff)


def three_members(text):
    """The text cut in three, the middle member an empty stream."""
    a = len(text) // 2
    return _member(text[:a], 8) + _member(b"", 4 | 16) + _member(text[a:], 2)


def streams():
    """variant -> (gzip bytes, text)"""
    if not _cache:
        t = edge_text()
        til = open(TILAPIA_FA, "rb").read()
        _cache.update({
            "l6": (gz(t), t), "l1": (gz(t, 1), t), "stored": (gz(t, 0), t), "fixed": (gz(t, 6, 8, zlib.Z_FIXED), t),
            "mem1": (gz(t, 6, 1), t), "three": (three_members(t), t), "tilapia": (gz(til), til)})
    return _cache


def files(datadir):
    """variant -> path of the .fa.gz, plus "plain" and "tilapia_plain" (written once)."""
    d = os.path.join(str(datadir), "fasta_gzip")
    paths = {v: os.path.join(d, f"{v}.fa.gz") for v in ALL_VARIANTS}
    paths["plain"] = os.path.join(d, "edge.fa")
    paths["tilapia_plain"] = TILAPIA_FA
    if not os.path.isdir(d):
        os.makedirs(d + ".tmp", exist_ok=True)
        for v, (s, _) in streams().items():
            with open(os.path.join(d + ".tmp", f"{v}.fa.gz"), "wb") as f:
                f.write(s)
        with open(os.path.join(d + ".tmp", "edge.fa"), "wb") as f:
            f.write(edge_text())
        os.rename(d + ".tmp", d)
    return paths


def plain_of(variant):
    return "tilapia_plain" if variant == "tilapia" else "plain"
