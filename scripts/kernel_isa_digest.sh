#!/bin/bash
# bash scripts/kernel_isa_digest.sh [FILE.hip ...]   (default: every .hip under lvc_amd/csrc that includes conv_common.h)
# Compiles each file's gfx950 device assembly with the library's flags and prints, per kernel,
#   file  kernel-name  sha256  vgpr sgpr vgpr_spill sgpr_spill lds scratch kernarg
# sha256 is over the kernel's instruction stream (label to end of function; comment lines and comment tails stripped).
# Two trees compute the same device code iff their outputs are equal: run it before and after a refactor and diff.
# KEEP_ASM=dir keeps the .s files.
set -euo pipefail
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
root=$(cd "$(dirname "$0")/.." && pwd)
csrc=$root/lvc_amd/csrc
exact=$(sed -n 's/^EXACT_SRCS *= *//p' "$csrc/Makefile")
if [ $# -eq 0 ]; then set -- $(cd "$csrc" && grep -l '"conv_common.h"' *.hip | sort); fi
tmp=${KEEP_ASM:-$(mktemp -d)}
mkdir -p "$tmp"
[ -n "${KEEP_ASM:-}" ] || trap 'rm -rf "$tmp"' EXIT
for f in "$@"; do
  f=$(basename "$f")
  extra=""
  case " $exact " in *" $f "*) extra="-ffp-contract=off -fno-fast-math" ;; esac
  "$HIPCC" --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-function $extra --cuda-device-only -S "$csrc/$f" -o "$tmp/${f%.hip}.s"
  python3 - "$f" "$tmp/${f%.hip}.s" <<'EOF'
import hashlib, re, sys
name, path = sys.argv[1], sys.argv[2]
lines = open(path).read().split("\n")
# instruction stream of every function symbol: from its label to its .Lfunc_end
body, cur = {}, None
for ln in lines:
    s = ln.split(";", 1)[0].rstrip() if '"' not in ln else ln.rstrip()
    if not s.strip() or re.match(r"\s*\.(file|ident)\b", s):
        continue
    m = re.match(r"^([A-Za-z_][\w$.]*):\s*$", s)
    if cur is None and m and not m.group(1).startswith(".L"):
        cur = m.group(1); body[cur] = []
        continue
    if cur is not None:
        if re.match(r"^\.Lfunc_end\d+:", s):
            cur = None
        else:
            body[cur].append(s.strip())
# metadata block (amdgpu_metadata YAML at the end of the file): one entry per kernel
keys = [".vgpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".group_segment_fixed_size",
        ".private_segment_fixed_size", ".kernarg_segment_size"]
meta, ent = {}, None
for ln in lines[lines.index("\t.amdgpu_metadata") if "\t.amdgpu_metadata" in lines else len(lines):]:
    t = ln.strip()
    if t.startswith("- .agpr_count:") or t.startswith("- .args:"):
        ent = {}
    m = re.match(r"-?\s*(\.[a-z_]+):\s*(\S+)$", t)
    if ent is not None and m:
        if m.group(1) == ".name" and ln.startswith("    .name:"):
            meta[m.group(2)] = ent
        elif m.group(1) in keys and ln.startswith("    "):
            ent[m.group(1)] = m.group(2)
for k in sorted(meta):
    if k not in body:
        sys.exit(f"{name}: kernel {k} has metadata but no body")
    h = hashlib.sha256("\n".join(body[k]).encode()).hexdigest()
    print(name, k, h, *[meta[k].get(x, "?") for x in keys])
# device functions that were not inlined are part of the device code too
for k in sorted(set(body) - set(meta)):
    if body[k] and any(re.match(r"[sv]_|buffer_|global_|ds_|flat_", x) for x in body[k]):
        print(name, k, hashlib.sha256("\n".join(body[k]).encode()).hexdigest(), "(function)")
EOF
done
