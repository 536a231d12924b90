# sha256 of the gfx950 device code (.text of the embedded code object) of every object of the product build:
#   bash tools/device_code_digest.sh > /tmp/a.txt ; (edit sources, python -m iaf_amd.build) ; bash tools/device_code_digest.sh | diff /tmp/a.txt -
# An experiment switch (#ifdef IAF_EXP_*) must leave every line unchanged: that is how this round kept staging experiments
# after the GPU budget was spent without touching what the GPU suite had verified.
#
# When code moves between translation units the units' own digests change; then compare kernel by kernel:
#   bash tools/device_code_digest.sh --kernels iaf_engine [iaf_model_ops ...]
# prints one line per device function of the named objects, sorted by symbol: the sha256 of its disassembly with the addresses and
# encodings stripped (branch operands are relative) and without the padding behind it, and the symbol.  The union over the units a
# move touches must not change.  Two kinds of function can still differ after a pure move, so read the diff of each that does:
#   * one that addresses a symbol relative to its own pc (s_getpc_b64): the literal is the distance between the two, which moves;
#   * one that calls an inline helper with an argument the compiler folds per translation unit.  __shfl_down(v, o, 64) is the case
#     met here: in a unit where EVERY caller of the HIP header's __shfl_down passes width 64 the width is folded into the helper
#     before it is inlined and the lane-index arithmetic in front of ds_bpermute comes out in another (equivalent) form than in a
#     unit that also has a default-width caller ("Source").
L=/opt/rocm/lib/llvm/bin
T=$(mktemp -d)
OBJ=${IAF_OBJ_DIR:-"$(dirname "$0")"/../iaf_amd/_lib/obj}    # IAF_OBJ_DIR: the objects of another build (the parent's, say)
unbundle() {   # $1 = object name without .o  ->  $T/$1.co
  cp $OBJ/$1.o $T/$1.o
  $L/llvm-objcopy --dump-section .hip_fatbin=$T/$1.bin $T/$1.o $T/$1.copy.o 2>/dev/null &&
  $L/clang-offload-bundler --type=o --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --input=$T/$1.bin --output=$T/$1.co --unbundle 2>/dev/null
}
if [ "$1" = "--kernels" ]; then
  shift
  for n in "$@"; do
    unbundle $n || { echo "no device code in $n" >&2; continue; }
    # a function starts at "<address> <symbol>:"; an instruction's address and encoding sit in its trailing // comment
    $L/llvm-objdump -d $T/$n.co | awk -v dir=$T -v unit=$n '
      /^[0-9a-f]+ <.*>:$/ { if (k) close(f); held = ""; k++; f = dir "/" unit "." k ".fn"; sub(/^[0-9a-f]+ </, ""); sub(/>:$/, ""); print > (f ".name"); close(f ".name"); next }
      k { sub(/[ \t]*\/\/.*$/, "")
          # padding up to the next function (a long run of it is printed as "..."): layout, not code
          if ($0 ~ /^[ \t]*(s_nop 0|s_code_end|\.\.\.)?[ \t]*$/) { held = held $0 "\n"; next }
          printf "%s", held > f; held = ""; print > f }'
    for f in $T/$n.*.fn; do
      [ -e "$f" ] && echo "$(sha256sum < $f | cut -c1-16)  $(cat $f.name)"
    done
  done | sort -k2
  rm -rf $T
  exit 0
fi
for o in $OBJ/*.o; do
  n=$(basename $o .o)
  unbundle $n &&
  $L/llvm-objcopy -O binary --only-section=.text $T/$n.co $T/$n.text &&
  echo "$(sha256sum < $T/$n.text | cut -c1-16)  $n"
done
rm -rf $T
