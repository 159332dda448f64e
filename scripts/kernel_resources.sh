#!/bin/bash
# Register / LDS / scratch use of every kernel in one translation unit of libmdx (no GPU needed):
#   scripts/kernel_resources.sh mdx_rdf [pattern]
# Recompiles the unit with --save-temps in a scratch directory, with the flags the Makefile gives it (the contract
# units are built with contraction and SLP vectorisation off), and reads the code-object notes.  Every field is booked
# on the .name of its own metadata entry: an entry starts at "  - " and lists its fields in alphabetical order, so
# some stand before the name and some after it.
set -e
unit=${1:-mdx_rdf}
pat=${2:-.}
root=$(cd "$(dirname "$0")/.." && pwd)
mk="$root/mdhelper_amd/csrc/Makefile"
extra=""
if sed -n 's/^CONTRACT_UNITS *= *//p' "$mk" | tr ' ' '\n' | grep -qx "$unit"; then
    extra=$(sed -n 's/^RDF_FLAGS *= *//p' "$mk")
fi
tmp=$(mktemp -d)
cd "$tmp"
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -I"$root/include" $extra --save-temps \
    -c "$root/mdhelper_amd/csrc/$unit.hip" -o out.o >/dev/null 2>&1
awk '
    function flush() { if (name != "") print name fields; name = ""; fields = "" }
    /^  - \./ { flush(); sub(/^  - /, "    ") }
    /^    \.name:/ { name = $2 }
    /^    \.(vgpr_count|sgpr_count|vgpr_spill_count|sgpr_spill_count|group_segment_fixed_size|private_segment_fixed_size):/ {
        fields = fields " " $1 $2
    }
    /^\.\.\.$/ { flush() }
    END { flush() }
' ./*gfx950*.s | grep -E "$pat" | sort
rm -rf "$tmp"
