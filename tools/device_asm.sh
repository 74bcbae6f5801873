#!/bin/bash
# Device-side assembly of every kernel object, compiled as the Makefile compiles it: tools/device_asm.sh OUTDIR [TREE]
# Each command is the one `make -nB build/NAME.o` prints (so the flags cannot drift from the Makefile's), with
# `-c -o build/NAME.o` replaced by `--cuda-device-only -S -o OUTDIR/NAME.s`.  Compare two trees with `diff -r` on their
# OUTDIRs (paths are relative to openwhisk_amd/, so both spell file names alike); identical output is the evidence
# that a host-only change left the kernels alone.  The compilation-unit id clang derives from a hash of each source
# file (__hip_cuid_<hash>, one byte of data that no kernel reads) is replaced by a fixed name: it changes with any
# edit of the file, a comment or an #include included.
set -e -o pipefail
out=$(realpath -m "$1")
cd "${2:-$(dirname "$0")/..}/openwhisk_amd"
mkdir -p "$out"
for f in csrc/*.hip; do
    b=$(basename "$f" .hip)
    make -nB "build/$b.o" | grep -- " -c -o build/$b.o " | sed "s# -c -o build/$b.o # --cuda-device-only -S -o $out/$b.s #"
done | xargs -P "${JOBS:-4}" -I{} sh -c {}
sed -i -E 's/__hip_cuid_[0-9a-f]+/__hip_cuid_X/g' "$out"/*.s
(cd "$out" && sha256sum *.s)
