#!/bin/bash
# compares the gfx950 code objects of two builds: tools/disasm_diff.sh <obj dir A> <obj dir B>
# (obj dir = PMAF_OUT/obj of csrc/build.sh). Every kernel object present in both directories is disassembled
# (tools/disasm.sh) and compared without the `file format` line, which carries a temp-file path: prints `identical` or the
# number of differing lines per object. The one artefact to expect between identical sources under another name:
# s_add_u32 literals of PC-relative .rodata addresses (NOTES.md 1, "Comparing code objects across a source change").
set -e
[ $# -eq 2 ] || { echo "usage: $0 <obj dir A> <obj dir B>" >&2; exit 2; }
HERE=$(cd "$(dirname "$0")" && pwd)
T=$(mktemp -d)
trap 'rm -rf "$T"' EXIT
for a in "$1"/*.o; do
  n=$(basename "$a" .o)
  b="$2/$n.o"
  case "$n" in host*|shard) continue ;; esac   # host objects: no code object
  [ -f "$b" ] || continue
  "$HERE/disasm.sh" "$a" "$T/a.s"
  "$HERE/disasm.sh" "$b" "$T/b.s"
  d=$(diff <(grep -v 'file format' "$T/a.s") <(grep -v 'file format' "$T/b.s") | grep -c '^[<>]' || true)
  if [ "$d" = 0 ]; then echo "$n: identical"; else echo "$n: $d differing lines"; fi
done
