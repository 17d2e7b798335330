#!/bin/bash
# usage: resources.sh file.hip  -- prints kernel name, VGPRs, AGPRs, scratch bytes, occupancy, LDS, compiled with the Makefile's flags
# for the files in its STRICT list (-fno-slp-vectorize -ffp-contract=off; the others differ by -ffp-contract alone)
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -munsafe-fp-atomics -fno-slp-vectorize -ffp-contract=off -Rpass-analysis=kernel-resource-usage -c "$1" -o /tmp/_res.o 2>&1 \
 | grep -E "Function Name:| VGPRs:| AGPRs:|ScratchSize|Occupancy|LDS Size" \
 | sed -E 's/^.*remark: +//; s/ \[-Rpass.*//' \
 | awk '/^Function Name/{if(n)print n, v, a, s, o, l; n=$3} /^VGPRs:/{v="vgpr="$2} /^AGPRs:/{a="agpr="$2} /^ScratchSize/{s="scratch="$NF} /^Occupancy/{o="occ="$NF} /^LDS Size/{l="lds="$NF} END{print n, v, a, s, o, l}' \
 | sed 's/_ZN12_GLOBAL__N_1//' | cut -c1-160
