#!/bin/bash
# usage: tools/render_isa_sha.sh [extra -D flags...]   -> sha256, kernel count and path of render.hip's gfx950 device assembly (no GPU needed)
# The __hip_cuid_<hash> symbol hashes the source text; with it normalised, a pure code move leaves the digest unchanged.  To compare with
# another commit, run that checkout's copy of this script (git worktree; copy the script in if the commit predates it) and diff the two files.
# The assembly (~15 MB) is left under ${TMPDIR:-/tmp} for that diff, its path is the last word printed: delete it when done.
cd "$(dirname "$0")/../sanerf-hq_amd/csrc"
out=$(mktemp -t render_isa.XXXXXX.s)
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -munsafe-fp-atomics \
  -fhip-fp32-correctly-rounded-divide-sqrt -fno-gpu-flush-denormals-to-zero -Wall -Wno-unused-function -Wno-pass-failed "$@" \
  -S --cuda-device-only render.hip -o "$out" || { rm -f "$out"; exit 1; }
sed -i -E 's/__hip_cuid_[0-9a-f]+/__hip_cuid_X/g' "$out"
echo "sha256=$(sha256sum "$out" | cut -d' ' -f1) kernels=$(grep -c '^[[:space:]]*\.amdhsa_kernel ' "$out") $out"
