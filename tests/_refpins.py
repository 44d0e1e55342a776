"""The reference's answers on the inputs of the bit-exactness tests, kept in tests/golden/ref_pins.json so that those
tests run without the reference tree: what its own objects (oracle/_ref: fft_radix2.c, g-l_dpss.c, avg.c, util.c,
wav_fmt.c) return, the fields of its glfer.h structs and the symbols its kept files take from the dropped ones.
Arrays are kept as SHA-256 of dtype, shape and bytes (the tests compare bit for bit), floats as float.hex.

Regenerate where the reference tree is present, after `make -C oracle ref REF=<tree>`:

    python tests/_refpins.py <tree>
"""
import hashlib
import json
import os
import re
import struct
import sys

import numpy as np

PINS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_pins.json")

FFT_NS = [2, 4, 8, 16, 64, 512, 1024, 4096, 16384]
DPSS_CASES = [(256, 2, 1.5), (1024, 4, 2.5), (4096, 4, 2.5), (4096, 7, 4.0), (16384, 8, 4.5)]
AVG_MODES = ["plain", "sumextreme", "sumavg"]
WAV_CASES = [(16, 2 * 300, 512), (16, 2 * 300 + 1, 512), (8, 77, 512), (16, 0, 256), (8, 1, 102), (16, 2 * 5, 1024)]
# the files the compatibility library replaces when glfer is relinked against it (bell-p-w.c is not part of the program)
DROPPED = ["fft.c", "fft_radix2.c", "mtm.c", "g-l_dpss.c", "avg.c", "hparma.c", "lmp.c", "wav_fmt.c"]


def sha(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(("%s%s" % (a.dtype.str, a.shape)).encode() + a.tobytes()).hexdigest()


def num(v):
    """A scalar as the pins keep it: floats bit for bit (every NaN alike), integers as they are."""
    return v if isinstance(v, (int, np.integer)) and not isinstance(v, bool) else float(v).hex()


def load():
    with open(PINS) as f:
        return json.load(f)


# ---- the inputs (seeded; the pins hold a hash of each so that a changed generator is told apart from a changed oracle)

def fft_inputs(n):
    rng = np.random.default_rng(n)
    return [rng.standard_normal(n).astype(np.float32) for _ in range(3)]


def bessel_inputs():
    return np.linspace(0, 12, 97)


def svd_input():
    return np.random.default_rng(1).standard_normal((128, 33)).astype(np.float32)


def avg_inputs():
    """14 rows of 513 bins, each updated over bins 10..400 with max0 alternating."""
    rng = np.random.default_rng(5)
    return [(rng.random(513) ** 4).astype(np.float32) for _ in range(14)]


def avg_step(r):
    """One update's result (return value, averaged row, peak bin, variance) as the pins keep it."""
    return [num(r[0]), sha(r[1]), num(r[2]), num(r[3])]


def wav_pcm(bits, extra_bytes, hop):
    rng = np.random.default_rng(bits + extra_bytes)
    return rng.integers(0, 256, 7 * hop * (bits // 8) + extra_bytes, dtype=np.uint8)


def remove_mean(blk):
    """The estimator's in-place mean removal (fft.c:93-95), applied to each block the reader hands out."""
    blk -= np.float32(blk.sum(dtype=np.float32) / np.float32(blk.size))


def wav_key(bits, extra_bytes, hop):
    return "%d-%d-%d" % (bits, extra_bytes, hop)


def struct_fields(text, name):
    """The (type, name) list of `typedef struct { ... } name;` in C source text, GTK pointers as void *."""
    body = re.search(r"typedef struct\s*\{([^}]*)\}\s*" + name + r"\s*;", re.sub(r"/\*.*?\*/", "", text, flags=re.S), re.S).group(1)
    out = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        m = re.match(r"(.*?)(\**)\s*(\w+)$", decl)
        typ, ptr, ident = m.group(1).strip(), m.group(2), m.group(3)
        if ptr and typ in ("GtkWidget", "GtkTooltips", "void"):
            typ = "void"
        out.append((typ + ptr, ident))
    return out


# ---- the generator

def _lp64_wav(path, pcm_bytes, bits, rate):
    """A header the reference's open_wav_file() parses correctly on an LP64 host: its struct uses u_long, so it is 88
    bytes with format at 40, sample_fq at 48 and bit_p_spl at 66 (wav_fmt.h:34-52)."""
    hd = bytearray(88)
    hd[0:4] = b"RIFF"
    struct.pack_into("<H", hd, 40, 1)          # format = PCM
    struct.pack_into("<H", hd, 42, 1)          # modus = mono
    struct.pack_into("<Q", hd, 48, rate)       # sample_fq
    struct.pack_into("<H", hd, 64, bits // 8)  # byte_p_spl
    struct.pack_into("<H", hd, 66, bits)       # bit_p_spl
    with open(path, "wb") as f:
        f.write(bytes(hd))
        f.write(pcm_bytes)


def _kept_needs(tree):
    """Every non-static function or object the dropped files define that a kept file (glfer.c source.c g_main.c
    g_options.c ...) names."""
    kept = [f for f in os.listdir(tree) if f.endswith(".c") and f not in DROPPED and f != "bell-p-w.c"]
    defined = set()
    for f in DROPPED:
        for line in open(os.path.join(tree, f), errors="replace"):
            m = re.match(r"^(?!static)[A-Za-z_][\w \*]*?\**\b(\w+)\s*(\(|\[\]\s*=|=)", line)
            if m and not line.rstrip().endswith(";") or (m and "=" in line):
                defined.add(m.group(1))
    kept_text = " ".join(open(os.path.join(tree, f), errors="replace").read() for f in kept)
    return sorted(s for s in defined if re.search(r"\b" + s + r"\b", kept_text) and s not in ("main", "opt", "glfer"))


def generate(tree):
    import tempfile
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import oracle as O
    ref = O.Ref()
    pins = {"fft": {}, "dpss": {}, "avg": {}, "wav": {}}
    for n in FFT_NS:
        pins["fft"][str(n)] = [{"in": sha(x), "out": sha(ref.rfft_halfcomplex(x))} for x in fft_inputs(n)]
    for n, kmax, nw in DPSS_CASES:
        err, v, s = ref.dpss(n, kmax, nw)
        pins["dpss"]["%d-%d-%s" % (n, kmax, nw)] = {"err": err, "v": sha(v), "s": sha(s)}
    pins["bessel_i0"] = [num(ref.bessel_i0(x)) for x in bessel_inputs()]
    a = svd_input()
    rc, u, s, q = ref.svd(a)
    pins["svd"] = {"in": sha(a), "rc": rc, "u": sha(u), "s": sha(s), "q": sha(q)}
    rows = avg_inputs()
    pins["avg_in"] = sha(np.stack(rows))
    for mode in AVG_MODES:
        av = ref.averager(1024, 4)
        pins["avg"][mode] = [avg_step(av.update(mode, psd, 10, 400, max0=f % 2, n=513)) for f, psd in enumerate(rows)]
    with tempfile.TemporaryDirectory() as d:
        for bits, extra, hop in WAV_CASES:
            pcm = wav_pcm(bits, extra, hop)
            path = os.path.join(d, "lp64.wav")
            _lp64_wav(path, pcm.tobytes(), bits, 8000)
            case = {"in": sha(pcm)}
            for label, mutate in (("as_read", None), ("mean_removed", remove_mean)):
                blocks, speed = ref.wav_blocks(path, hop, mutate)
                case[label] = {"speed": speed, "blocks": [sha(b) for b in blocks]}
            pins["wav"][wav_key(bits, extra, hop)] = case
    header = open(os.path.join(tree, "glfer.h")).read()
    pins["glfer_h"] = {name: struct_fields(header, name) for name in ("opt_t", "glfer_t")}
    pins["kept_files_need"] = _kept_needs(tree)
    with open(PINS, "w") as f:
        json.dump(pins, f, indent=1)
        f.write("\n")
    print("wrote", PINS)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    generate(sys.argv[1])
