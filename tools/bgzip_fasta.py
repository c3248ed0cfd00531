#!/usr/bin/env python3
"""bgzip a FASTA (or any file) with zlib alone: BGZF blocks of 65,280 payload
bytes and the 28-byte EOF block, as `bgzip` writes them.

    python tools/bgzip_fasta.py genome.fa            -> genome.fa.gz
    python tools/bgzip_fasta.py genome.fa out.fa.gz -l 6
    python tools/bgzip_fasta.py genome.fa --device 0    (on the GPU: grom_amd.bgzf_compress, also genome.fa.gz.gzi)
"""
import argparse
import os
import struct
import sys
import zlib

PAYLOAD = 65280


def block(payload, level):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    z = c.compress(payload) + c.flush()
    if len(z) + 26 > 65536:  # does not happen at 65,280 payload bytes; stored as it is
        c = zlib.compressobj(0, zlib.DEFLATED, -15)
        z = c.compress(payload) + c.flush()
    return (struct.pack("<4BI2BH2B2H", 0x1f, 0x8b, 8, 4, 0, 0, 0xff, 6, 66, 67, 2, len(z) + 25) + z +
            struct.pack("<II", zlib.crc32(payload), len(payload)))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("src")
    ap.add_argument("dst", nargs="?")
    ap.add_argument("-l", "--level", type=int, default=1)
    ap.add_argument("--device", type=int, default=None, metavar="N",
                    help="compress on GPU N with the library's DEFLATE kernels (-l does not apply)")
    a = ap.parse_args()
    dst = a.dst or a.src + ".gz"
    if a.device is not None:
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        import grom_amd
        st = grom_amd.bgzf_compress(a.src, dst, device=a.device)
        print(f"{dst}: {st['blocks']} blocks, {st['in_bytes']} -> {st['out_bytes']} bytes on device {a.device}")
        return
    n = 0
    with open(a.src, "rb") as f, open(dst, "wb") as g:
        while True:
            p = f.read(PAYLOAD)
            if not p:
                break
            g.write(block(p, a.level))
            n += 1
        g.write(block(b"", a.level))
    print(f"{dst}: {n} blocks")


if __name__ == "__main__":
    main()
