"""The ND2 files of the reference's test data (RT/data) as a small golden vector:

    python tools/make_golden_nd2.py <directory holding the reference's example-*.nd2 files>

Writes tests/golden/nd2_fixture_files.npz for tests/test_host_api.py: every file byte for byte, except that the pixel
payload of each ``ImageDataSeq|N!`` chunk (after its 8-byte frame header) is zeroed.  Chunk map, attributes and
metadata are untouched, so the parser meets the files' real layout; the pixels of config 1 are pinned separately in
tests/golden/nd2_multichannel.npz.  The files are stored concatenated (``data``, ``names``, ``sizes``) in an
LZMA-compressed archive, which numpy reads like any .npz.
"""
import os
import struct
import sys
import zipfile

import numpy as np

NAMES = ("example-multichannel.nd2", "example-pbmc.nd2", "example-cerevisiae.nd2", "example-timelapse.nd2",
         "example-zstack.nd2")
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden",
                   "nd2_fixture_files.npz")
CHUNK_MAGIC = 0x0ABECEDA


def zero_pixels(blob: bytes) -> bytes:
    """Walk the chunks one after the other (padding between them is skipped) and zero the image payloads."""
    b = bytearray(blob)
    pos = 0
    while pos + 16 <= len(b):
        magic, nlen, dlen = struct.unpack_from("<IIQ", b, pos)
        if magic != CHUNK_MAGIC:
            pos += 1
            continue
        name = bytes(b[pos + 16: pos + 16 + nlen]).split(b"\x00")[0]
        data = pos + 16 + nlen
        if name.startswith(b"ImageDataSeq|"):
            b[data + 8: data + dlen] = bytes(dlen - 8)
        pos = data + dlen
    return bytes(b)


def main():
    src = sys.argv[1]
    blobs = [zero_pixels(open(os.path.join(src, n), "rb").read()) for n in NAMES]
    arrays = {"names": np.array(NAMES), "sizes": np.array([len(x) for x in blobs], np.int64),
              "data": np.frombuffer(b"".join(blobs), np.uint8)}
    with zipfile.ZipFile(OUT, "w", compression=zipfile.ZIP_LZMA) as zf:
        for key, a in arrays.items():
            with zf.open(key + ".npy", "w") as f:
                np.lib.format.write_array(f, a, allow_pickle=False)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
