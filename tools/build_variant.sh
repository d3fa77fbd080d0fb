#!/bin/bash
# Build librhp.so from the working tree with extra compile flags, for same-box
# A/B runs (tools/ab_libs.py):
#   tools/build_variant.sh <tag> -DRHP_ROW_STRIDE=260 ...  ->  libreactorng_amd/librhp_x_<tag>.so
set -e
tag=$1; shift
make -C "$(git rev-parse --show-toplevel)/libreactorng_amd/csrc" variant TAG="$tag" XFLAGS="$*"
echo "built libreactorng_amd/librhp_x_$tag.so ($*)"
