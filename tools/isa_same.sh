#!/bin/bash
# Are the device instructions of UNIT... in the working tree those of git revision REV?
#   bash tools/isa_same.sh HEAD~1 lrt_temporal lrt_rectify
# REV's csrc and include are archived into a temporary directory; `make isa U=<unit>` runs there and
# in the working tree; directive lines, comment lines, trailing comments and the lines that only name
# a symbol (labels, which carry the mangled kernel names) are dropped from both .s files and the rest
# is diffed. Per unit: the count of differing lines and the two resource tables (the compiler's
# kernel-resource-usage remarks). Exit status 1 if any unit differs.
set -e -o pipefail
[ $# -ge 2 ] || { echo "usage: $0 REV UNIT..." >&2; exit 2; }
rev=$1; shift
root=$(cd "$(dirname "$0")/.." && pwd)
tmp=$(mktemp -d)
trap 'rm -rf "$tmp"' EXIT
git -C "$root" archive "$rev" learnraytracing_amd/csrc include | tar -x -C "$tmp"

# the instruction lines of $1
strip() {
  sed -e 's/[[:space:]]*;.*$//' -e 's,[[:space:]]*//.*$,,' -e 's/[[:space:]]*$//' "$1" |
    grep -v -E '^[[:space:]]*(\.|$)' | grep -v -E '^[^[:space:]]+:$' || true
}
# the resource table of a `make isa` log: one line per kernel
table() {
  grep -E 'remark: .*(Function Name|VGPRs:|SGPRs:|ScratchSize|Occupancy|LDS Size)' "$1" |
    sed -e 's/^.*remark: *//' -e 's/ \[-Rpass-analysis.*$//' -e 's/ \[[a-z/]*\]//' |
    awk '/Function Name/ { if (line) print line; sub(/Function Name: /, ""); line = "  " $0; next }
         { line = line ", " $0 } END { if (line) print line }'
}

bad=0
for u in "$@"; do
  for side in "$tmp" "$root"; do
    dir=$side/learnraytracing_amd/csrc
    make -s -C "$dir" isa U="$u" >"$tmp/$u.$( [ "$side" = "$tmp" ] && echo old || echo new ).log" 2>&1 ||
      { echo "$u: make isa failed in $dir" >&2; tail -20 "$tmp/$u."*.log >&2; exit 2; }
  done
  strip "$tmp/learnraytracing_amd/csrc/$u.s" >"$tmp/$u.old.txt"
  strip "$root/learnraytracing_amd/csrc/$u.s" >"$tmp/$u.new.txt"
  rm -f "$root/learnraytracing_amd/csrc/$u.s"
  n=$(diff "$tmp/$u.old.txt" "$tmp/$u.new.txt" | grep -c '^[<>]' || true)
  echo "$u: $n differing lines of $(wc -l <"$tmp/$u.new.txt") ($rev against the working tree)"
  echo " $rev:"; table "$tmp/$u.old.log"
  echo " working tree:"; table "$tmp/$u.new.log"
  [ "$n" -eq 0 ] || bad=1
done
exit $bad
