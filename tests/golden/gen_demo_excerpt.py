"""Generates tests/golden/demo_excerpt.mp4: the first 176 access units of the reference's demo video demo/1m.mp4 (its key
frame and the P / B pictures behind it, 0.47 MB) as an MP4 of their own, for the host tests of the container / H.264 front
end (tests/test_host_h264.py, tests/test_gst_elements.py, tests/helpers/san_fuzz.py).  The cut closes the output order:
the 176 access units are the first 176 output pictures.  The file keeps its layout -- ftyp, free, mdat, then moov -- with
the sample tables (stts, ctts, stss, stsz, stsc, stco) and the durations (mvhd, tkhd, elst, mdhd) cut to the kept samples.  Run once, where the
reference tree is present: python tests/golden/gen_demo_excerpt.py /path/to/reference/demo/1m.mp4"""
import os
import struct
import sys

N = 176
CONTAINERS = {b"moov", b"trak", b"mdia", b"minf", b"stbl", b"edts"}


def boxes(d, o, end):
    while o < end:
        size, kind = struct.unpack(">I4s", d[o:o + 8])
        assert size >= 8, "64-bit box sizes are not expected in this file"
        yield kind, d[o + 8:o + size]
        o += size


def box(kind, body):
    return struct.pack(">I4s", 8 + len(body), kind) + body


def runs(values):
    out = []
    for v in values:
        if out and out[-1][1] == v:
            out[-1][0] += 1
        else:
            out.append([1, v])
    return out


def main(src, dst):
    d = open(src, "rb").read()
    top = list(boxes(d, 0, len(d)))
    assert [k for k, _ in top][:4] == [b"ftyp", b"free", b"mdat", b"moov"]
    stbl = {}

    def find(body, path):
        for k, b in boxes(body, 0, len(body)):
            if k == path[0]:
                return b if len(path) == 1 else find(b, path[1:])
    moov = top[3][1]
    body = find(moov, [b"trak", b"mdia", b"minf", b"stbl"])
    for k, b in boxes(body, 0, len(body)):
        stbl[k] = b
    total = struct.unpack(">I", stbl[b"stsz"][8:12])[0]
    sizes = struct.unpack(f">{total}I", stbl[b"stsz"][12:12 + 4 * total])
    (n_stts,) = struct.unpack(">I", stbl[b"stts"][4:8])
    deltas = [dl for i in range(n_stts) for c, dl in [struct.unpack(">II", stbl[b"stts"][8 + 8 * i:16 + 8 * i])] for _ in range(c)]
    (n_ctts,) = struct.unpack(">I", stbl[b"ctts"][4:8])
    version = stbl[b"ctts"][0]
    offs = [o for i in range(n_ctts) for c, o in [struct.unpack(">I" + ("i" if version else "I"), stbl[b"ctts"][8 + 8 * i:16 + 8 * i])]
            for _ in range(c)]
    (n_stss,) = struct.unpack(">I", stbl[b"stss"][4:8])
    sync = struct.unpack(f">{n_stss}I", stbl[b"stss"][8:8 + 4 * n_stss])
    (n_stsc,) = struct.unpack(">I", stbl[b"stsc"][4:8])
    stsc = [struct.unpack(">III", stbl[b"stsc"][8 + 12 * i:20 + 12 * i]) for i in range(n_stsc)]
    (n_stco,) = struct.unpack(">I", stbl[b"stco"][4:8])
    stco = struct.unpack(f">{n_stco}I", stbl[b"stco"][8:8 + 4 * n_stco])
    assert len(deltas) == len(offs) == total and [e[0] for e in stsc] == list(range(1, n_stsc + 1)) and all(e[1] > 0 for e in stsc)
    # the chunks that hold the first N samples; the last of them is cut to what it holds of those
    per_chunk = [e[1] for e in stsc]
    n_chunks = next(i + 1 for i in range(n_stsc) if sum(per_chunk[:i + 1]) >= N)
    kept = per_chunk[:n_chunks - 1] + [N - sum(per_chunk[:n_chunks - 1])]
    for c in range(n_chunks):                              # the kept samples sit back to back in mdat, chunk after chunk
        assert stco[c] == stco[0] + sum(sizes[:sum(per_chunk[:c])])
    mdat_start = (8 + len(top[0][1])) + (8 + len(top[1][1])) + 8      # first byte of mdat's payload
    assert stco[0] == mdat_start                                         # ... is the first sample's
    mdat = d[mdat_start:mdat_start + sum(sizes[:N])]
    media_dur = sum(deltas[:N])
    old_media_dur = sum(deltas)

    def tables():
        b = {}
        b[b"stts"] = bytes(4) + struct.pack(">I", len(runs(deltas[:N]))) + b"".join(struct.pack(">II", c, v) for c, v in runs(deltas[:N]))
        ct = runs(offs[:N])
        b[b"ctts"] = stbl[b"ctts"][:4] + struct.pack(">I", len(ct)) + b"".join(struct.pack(">I" + ("i" if version else "I"), c, v) for c, v in ct)
        ks = [s for s in sync if s <= N]
        b[b"stss"] = bytes(4) + struct.pack(f">I{len(ks)}I", len(ks), *ks)
        b[b"stsz"] = bytes(4) + struct.pack(f">II{N}I", 0, N, *sizes[:N])
        b[b"stsc"] = bytes(4) + struct.pack(">I", n_chunks) + b"".join(struct.pack(">III", c + 1, kept[c], stsc[c][2]) for c in range(n_chunks))
        b[b"stco"] = bytes(4) + struct.pack(f">I{n_chunks}I", n_chunks, *stco[:n_chunks])
        return b
    new_tables = tables()

    def scaled(x):
        return x * media_dur // old_media_dur

    def rewrite(kind, body):
        if kind in CONTAINERS:
            return box(kind, b"".join(rewrite(k, b) for k, b in boxes(body, 0, len(body))))
        if kind in new_tables:
            return box(kind, new_tables[kind])
        if kind in (b"mvhd", b"tkhd", b"mdhd"):
            assert body[0] == 0, "version-0 headers expected"
            at = {b"mvhd": 16, b"tkhd": 20, b"mdhd": 16}[kind]
            (dur,) = struct.unpack(">I", body[at:at + 4])
            new = media_dur if kind == b"mdhd" else scaled(dur)
            return box(kind, body[:at] + struct.pack(">I", new) + body[at + 4:])
        if kind == b"elst":
            assert body[0] == 0 and struct.unpack(">I", body[4:8])[0] == 1
            (dur,) = struct.unpack(">I", body[8:12])
            return box(kind, body[:8] + struct.pack(">I", scaled(dur)) + body[12:])
        return box(kind, body)

    out = box(b"ftyp", top[0][1]) + box(b"free", top[1][1]) + box(b"mdat", mdat) + rewrite(b"moov", moov)
    open(dst, "wb").write(out)
    print(f"{dst}: {N} of {total} access units, {len(out)} bytes")


if __name__ == "__main__":
    main(sys.argv[1], os.path.join(os.path.dirname(os.path.abspath(__file__)), "demo_excerpt.mp4"))
