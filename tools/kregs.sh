#!/bin/bash
# registers / scratch / LDS of every kernel of the objects of a build directory (default: ulc-codec_amd/build), by its full
# demangled name; optional filter on the printed line
# usage: tools/kregs.sh [--isa] [build dir] [pattern]
#   --isa: a further column, the md5 of the kernel's disassembly with addresses, comments and symbol names stripped - two builds
#          whose kernel has the same instruction stream print the same hash.  --isa=DIR also leaves that text in DIR/<mangled name>.s
ISA=; ISADIR=
case "$1" in --isa) ISA=1; shift;; --isa=*) ISA=1; ISADIR=${1#--isa=}; shift;; esac
DIR=${1:-ulc-codec_amd/build}; PAT=${2:-.}; K=9; [ -n "$ISA" ] && K=11     # K: the field the name starts at
LLVM=/opt/rocm/lib/llvm/bin
T=$(mktemp -d); trap 'rm -rf $T' EXIT
[ -n "$ISADIR" ] && mkdir -p "$ISADIR"
for o in $DIR/ulcx_enc_wc.o $DIR/ulcx_enc_xf.o $DIR/ulcx_enc_xfa.o $DIR/ulcx_enc_psy.o $DIR/ulcx_enc_wr.o $DIR/ulcx_enc_ladder.o $DIR/ulcx_dec.o $DIR/ulcx_slots.o $DIR/ulcx_clips.o; do
  [ -f $o ] || continue
  objcopy -O binary --only-section=.hip_fatbin $o $T/fat.bin
  $LLVM/clang-offload-bundler --type=o --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --input=$T/fat.bin --output=$T/dev.co --unbundle 2>/dev/null || continue
  : > $T/isa.tsv
  if [ -n "$ISA" ]; then
    # one text per function: the label opens it; of a line, the address in front, a trailing comment and every <symbol+offset> go
    rm -rf $T/isa; mkdir $T/isa
    $LLVM/llvm-objdump -d --no-show-raw-insn $T/dev.co | awk -v d=$T/isa '
      /^[0-9a-f]+ <.*>:$/ { if (f) close(f); n = $2; gsub(/[<>:]/, "", n); f = d "/" n ".s"; next }
      f && NF { sub(/^[ \t]*[0-9a-f]+:[ \t]*/, ""); sub(/[ \t]*\/\/.*$/, ""); gsub(/<[^>]*>/, "<>"); print > f }'
    for f in $T/isa/*.s; do
      n=$(basename $f .s); printf '%s\t%s\n' "$n" "$(md5sum < $f | cut -c1-12)" >> $T/isa.tsv
      [ -n "$ISADIR" ] && cp $f "$ISADIR/$n.s"
    done
  fi
  $LLVM/llvm-readelf --notes $T/dev.co | awk -v isa=$T/isa.tsv '
    BEGIN { while ((getline l < isa) > 0) { split(l, a, "\t"); h[a[1]] = a[2] } }
    /\.name:/ {name=$2} /\.vgpr_count:/ {v=$2} /\.sgpr_count:/ {sg=$2} /\.private_segment_fixed_size:/ {p=$2} /\.group_segment_fixed_size:/ {l=$2}
    /\.wavefront_size:/ {printf "%s\tvgpr %3d sgpr %3d scratch %5d lds %6d%s\n", name, v, sg, p, l, (name in h) ? " isa " h[name] : ""}' |
    while IFS=$'\t' read -r n rest; do printf '%s  %s\n' "$rest" "$(c++filt "$n")"; done | grep -E "$PAT" | sort -k$K
done
