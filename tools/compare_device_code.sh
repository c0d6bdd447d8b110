#!/bin/bash
# Is the device code of two checkouts the same?  For every multi_stylegan_amd/csrc/*.hip of both trees: compile the device side
# only, with the flags of multi_stylegan_amd/build.py, to gfx950 assembly; drop the lines that carry no instructions (.file, .ident,
# debug-location directives, comments, blank lines) and rename the one symbol hipcc derives from the source file's PATH
# (__hip_cuid_<hash>, a one-byte marker object), which differs between two checkouts of identical sources; compare.  Same assembly = same ISA, registers, LDS and kernel-argument layout
# (the .amdhsa_ directives and the kernel metadata are part of the compared text), i.e. a host-only change.  Needs only hipcc.
#
#   tools/compare_device_code.sh <tree A> <tree B> [work dir]        exit status 0: identical for every file
set -u
A=${1:?usage: compare_device_code.sh <tree A> <tree B> [work dir]}
B=${2:?usage: compare_device_code.sh <tree A> <tree B> [work dir]}
WORK=${3:-$(mktemp -d)}
HIPCC=$(command -v hipcc || echo /opt/rocm/bin/hipcc)
JOBS=${JOBS:-8}
mkdir -p "$WORK/a" "$WORK/b"

emit() {    # <tree> <out dir>: one filtered .s per source file
    local tree=$1 out=$2
    ls "$tree"/multi_stylegan_amd/csrc/*.hip | xargs -P "$JOBS" -I{} sh -c \
        '"$0" -O3 -std=c++17 --offload-arch=gfx950 -Wno-unused-result --cuda-device-only -S "$1" -o "$2/$(basename "$1").raw.s" &&
         grep -v -E "^[[:space:]]*(;|//|\.file|\.ident|\.loc|\.cfi_|\.section[[:space:]]+\.debug|$)" "$2/$(basename "$1").raw.s" |
             sed -E "s/__hip_cuid_[0-9a-f]+/__hip_cuid_X/g" > "$2/$(basename "$1").s"' "$HIPCC" {} "$out"
}
emit "$A" "$WORK/a" || { echo "compile failed in $A"; exit 2; }
emit "$B" "$WORK/b" || { echo "compile failed in $B"; exit 2; }

status=0
names=$( (cd "$WORK/a" && ls *.hip.s; cd "$WORK/b" && ls *.hip.s) | sort -u)
for n in $names; do
    if [ ! -f "$WORK/a/$n" ] || [ ! -f "$WORK/b/$n" ]; then echo "ONLY ONE SIDE  $n"; status=1
    elif cmp -s "$WORK/a/$n" "$WORK/b/$n"; then echo "identical      $n ($(wc -l < "$WORK/a/$n") lines)"
    else echo "DIFFERENT      $n"; diff "$WORK/a/$n" "$WORK/b/$n" | head -20; status=1
    fi
done
echo "$(echo "$names" | wc -w) files, $([ $status = 0 ] && echo "device code identical" || echo "device code DIFFERS")"
exit $status
