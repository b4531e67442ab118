"""Turn the reference's data/sde_demo.bson (experiments/sde_toy_problem.jl:8-10) into the text fixtures tests/golden/sde_demo/{sde_data,
sde_data_vars}.txt: 2 x 30 float32 each, Julia column-major order, every value as its exact bit pattern and in decimal.

    python tools/bson_fixture.py <path to sde_demo.bson> [out_dir]

A minimal BSON reader for that one file, not a general one: documents (0x03), strings (0x02), binary (0x05), int64 (0x12), int32 (0x10),
booleans (0x08) and arrays (0x04), which is what BSON.jl writes for a Dict of Array{Float32,2} -- each array is a document
{tag: "array", type: {tag: "datatype", name: ["Core", "Float32"], params: []}, size: [rows, cols], data: <raw little-endian bytes>}.
"""
import hashlib
import os
import struct
import sys

import numpy as np


def _cstring(b, i):
    j = b.index(b"\x00", i)
    return b[i:j].decode(), j + 1


def _document(b, i):
    n = struct.unpack_from("<i", b, i)[0]
    end, i, out = i + n - 1, i + 4, {}
    while i < end:
        t = b[i]
        key, i = _cstring(b, i + 1)
        if t in (0x03, 0x04):
            m = struct.unpack_from("<i", b, i)[0]
            v = _document(b, i)
            if t == 0x04:
                v = [v[k] for k in sorted(v, key=int)]
            i += m
        elif t == 0x02:
            m = struct.unpack_from("<i", b, i)[0]
            v = b[i + 4:i + 4 + m - 1].decode()
            i += 4 + m
        elif t == 0x05:
            m = struct.unpack_from("<i", b, i)[0]
            v = bytes(b[i + 5:i + 5 + m])
            i += 5 + m
        elif t == 0x12:
            v = struct.unpack_from("<q", b, i)[0]
            i += 8
        elif t == 0x10:
            v = struct.unpack_from("<i", b, i)[0]
            i += 4
        elif t == 0x08:
            v = bool(b[i])
            i += 1
        else:
            raise ValueError(f"BSON element type 0x{t:02x} at byte {i}: not in the subset this reader knows")
        out[key] = v
    return out


def julia_array(d):
    """A BSON.jl array document -> (rows, cols, float32 values in column-major order)."""
    if d.get("tag") != "array" or d["type"].get("name") != ["Core", "Float32"]:
        raise ValueError("expected a BSON.jl Array{Float32}")
    size = [int(s) for s in d["size"]]
    vals = np.frombuffer(d["data"], dtype="<f4")
    if vals.size != int(np.prod(size)):
        raise ValueError("data length does not match size")
    return size, vals


def write_fixture(path, name, src_name, sha, size, vals):
    with open(path, "w") as f:
        f.write(f"# {name}: Array{{Float32,2}} of size {size[0]} x {size[1]} from {src_name} (sha256 {sha})\n")
        f.write("# one value per line in Julia column-major order (element (r, c) at line c * rows + r, 0-based): float32 bits as hex, decimal\n")
        f.write(f"# size {size[0]} {size[1]}\n")
        for v in vals:
            bits = struct.unpack("<I", struct.pack("<f", float(v)))[0]
            f.write(f"0x{bits:08x} {float(v)!r}\n")


def main(argv):
    src = argv[1]
    out = argv[2] if len(argv) > 2 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "sde_demo")
    raw = open(src, "rb").read()
    sha = hashlib.sha256(raw).hexdigest()
    doc = _document(raw, 0)
    os.makedirs(out, exist_ok=True)
    for key in ("sde_data", "sde_data_vars"):
        size, vals = julia_array(doc[key])
        write_fixture(os.path.join(out, key + ".txt"), key, os.path.basename(src), sha, size, vals)
        print(key, size, vals[:2])


if __name__ == "__main__":
    main(sys.argv)
