#!/bin/bash
# Developer helper: memory operations of the forward step's kernels in the device ISA of blobnet_mfma.hip (the Makefile's flags).
# Per kernel: counts of flat_* / global_load* / global_load_lds* / global_store*, scratch bytes and VGPRs, and for every s_barrier
# the s_waitcnt that stands in front of it (with nothing but scalar / fence instructions between), i.e. what a wave has to have
# received before it may arrive.  A FLAT load counts on lgkmcnt AND vmcnt, so `lgkmcnt(0)` in front of a barrier also waits for
# every flat load in flight; a GLOBAL load counts on vmcnt alone ("Weight loads are global loads").
# usage: tools/isa_mem_ops.sh [-k <regex of demangled kernel names>] [extra hipcc flags]
#   default kernels: the five launches of the carrier-frame step
OUT=${ISA_OUT:-/tmp/isa}
KRE='enc0p_mfma<|enc1_mfma<|enc23_mfma<|dec012_mfma<|dec3cc_rows_mfma<'
if [ "$1" = "-k" ]; then KRE=$2; shift 2; fi
mkdir -p "$OUT"
cd "$(dirname "$0")/../cova_amd/csrc" || exit 1
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
if [ -z "$ISA_FILE" ]; then
    ISA_FILE=$OUT/mfma.s
    $HIPCC -O3 -std=c++17 --offload-arch=gfx950 -fno-honor-nans -mllvm -pragma-unroll-threshold=1000000 -I../../include -I. \
        -S --cuda-device-only blobnet_mfma.hip -o "$ISA_FILE" "$@" 2>&1 | grep -E "error" -A5 | head -30
fi
CXXFILT=$(dirname "$(readlink -f "$HIPCC")")/../llvm/bin/llvm-cxxfilt
[ -x "$CXXFILT" ] || CXXFILT=c++filt
ISA_FILE=$ISA_FILE KRE=$KRE CXXFILT=$CXXFILT python3 - <<'PY'
import os, re, subprocess, collections
txt = open(os.environ["ISA_FILE"]).read()
kre = re.compile(os.environ["KRE"])
meta = {n: (int(sc), int(v)) for n, sc, v in re.findall(
    r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)", txt)}
names = list(meta)
dem = subprocess.run([os.environ["CXXFILT"]], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
dem = {n: re.sub(r"\(anonymous namespace\)::|^void |\(.*$", "", d) for n, d in zip(names, dem)}
# instructions that neither issue nor wait for memory: a wait counts as "in front of" a barrier across them
skip = re.compile(r"^(s_(?!waitcnt|barrier)\w+|v_(mov|readfirstlane|accvgpr)\w*|buffer_wbl2|buffer_inv)\b")
for n in names:
    if not kre.search(dem[n]):
        continue
    m = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end" % re.escape(n), txt, re.S | re.M)
    ins = [l.split(";")[0].strip() for l in m.group(1).split("\n")]
    ins = [l for l in ins if l and not l.startswith(".") and not l.endswith(":")]
    cnt = collections.Counter()
    for l in ins:
        op = l.split()[0]
        for k in ("flat_load", "flat_store", "flat_atomic", "global_load_lds", "global_load", "global_store", "scratch_"):
            if op.startswith(k):
                cnt[k] += 1
                break
    bars = []
    for i, l in enumerate(ins):
        if l != "s_barrier":
            continue
        j = i - 1
        while j >= 0 and skip.match(ins[j]):
            j -= 1
        bars.append(ins[j].replace("s_waitcnt ", "") if j >= 0 and ins[j].startswith("s_waitcnt") else "-")
    sc, vg = meta[n]
    print("%s" % dem[n])
    print("    flat_load %d  flat_store %d  flat_atomic %d | global_load %d  global_load_lds %d  global_store %d | scratch %d B (%d scratch ops)  vgpr %d"
          % (cnt["flat_load"], cnt["flat_store"], cnt["flat_atomic"], cnt["global_load"], cnt["global_load_lds"], cnt["global_store"],
             sc, cnt["scratch_"], vg))
    print("    s_barrier x %d, the wait in front of each ('-' = none): %s" % (len(bars), " | ".join(bars)))
PY
