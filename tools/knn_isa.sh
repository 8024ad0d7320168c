#!/bin/bash
# Emits the gfx950 ISA of filters.hip and prints the register / spill / scratch / LDS figures of the three kernels that hold the
# exact k-NN search (what profiles/knn_walk_isa.txt keeps), for this tree or for a checkout of another commit:
#   tools/knn_isa.sh [root of a tree] >> profiles/knn_walk_isa.txt
set -e
root="$(cd "${1:-$(dirname "$0")/..}" && pwd)"
cd "$(dirname "$0")/.."
out="$(mktemp -d)/filters.s"
trap 'rm -rf "$(dirname "$out")"' EXIT
hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -I"$root/include" -S --cuda-device-only -o "$out" "$root/realsense-pointcloud_amd/csrc/filters.hip" 2>/dev/null
echo "filters.hip of $(basename "$root"), hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off, $(hipcc --version | grep -m1 "HIP version")"
for k in k_knn_mean_distance k_knn_indices k_normals; do
    sym=$(grep -o "^_ZN5rsreg[0-9]*${k}E[A-Za-z0-9_]*:" "$out" | head -1 | tr -d :)
    lines=$(awk -v s="$sym:" '$1 == s {on = 1} on {n++} on && /s_endpgm/ {print n; exit}' "$out")
    # the kernel's record of the amdhsa.kernels metadata: from one "  - ." line to the next
    awk -v s="$sym" -v k="$k" -v lines="$lines" '
        function flush() { if (name == s) printf "  %s: vgpr_count %s, sgpr_count %s, vgpr_spill_count %s, sgpr_spill_count %s, private_segment_fixed_size %s, group_segment_fixed_size %s; lines of ISA %s\n", k, f["vgpr_count"], f["sgpr_count"], f["vgpr_spill_count"], f["sgpr_spill_count"], f["private_segment_fixed_size"], f["group_segment_fixed_size"], lines; name = "" }
        /^amdhsa.kernels:/ {meta = 1}
        meta && /^  - \./ {flush()}
        meta && /^(  - |    )\.[a-z_]+: / {key = $0; sub(/^[ -]+\./, "", key); sub(/:.*/, "", key); val = $0; sub(/^[^:]*: */, "", val); if (key == "name") name = val; else f[key] = val}
        END {flush()}' "$out"
done
