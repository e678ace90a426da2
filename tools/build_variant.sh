#!/usr/bin/env bash
# tuning build of the library: tools/build_variant.sh <name> <extra hipcc flags...>  ->  take_amd/variants/lib_<name>.so
# (selected at run time with TAKE_HIP_LIB=...; tools/variants.sh runs bench.py over several of them)
# The flags, sources and libraries are take_amd/csrc/Makefile's; the extra flags go in as EXTRA.
set -e
name="$1"; shift
root="$(cd "$(dirname "$0")/.." && pwd)"
mkdir -p "$root/take_amd/variants"
make -C "$root/take_amd/csrc" -B OUT="../variants/lib_$name.so" EXTRA="$*" 2>&1 | grep -E "error|spill|Scratch" || true
ls -la "$root/take_amd/variants/lib_$name.so"
