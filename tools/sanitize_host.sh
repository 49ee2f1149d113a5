#!/bin/bash
# The host-parallel C++ of round 6 (csrc/delaunay_nd.cpp, cell_faces.cpp, host_parallel.hpp) under AddressSanitizer +
# UBSan and under ThreadSanitizer, as stand-alone programs on a CPU (GPU sanitizers are not available on this pool).
#   tools/sanitize_host.sh > profiles/face_table_sanitizers_host.txt
# "8 16 1", "8 30 1", "8 30 8" and the nine disjoint cells are inputs whose face table fills its first set of slots
# completely (the grow-and-refill path of flooder_cell_faces); tests/host_pool_main.cpp throws inside parallel regions.
cd "$(dirname "$0")/.."
tmp=$(mktemp -d) || exit 1
trap 'rm -rf "$tmp"' EXIT
for san in address,undefined thread; do
  g++ -O1 -g -std=c++17 -pthread -fsanitize=$san -fno-omit-frame-pointer -o "$tmp/flooder_san" tools/sanitize_host_main.cpp \
      flooder_amd/csrc/delaunay_nd.cpp flooder_amd/csrc/cell_faces.cpp || exit 1
  g++ -O1 -g -std=c++17 -pthread -fsanitize=$san -fno-omit-frame-pointer -Iflooder_amd/csrc -o "$tmp/pool_san" \
      tests/host_pool_main.cpp || exit 1
  echo "== -fsanitize=$san"
  for cfg in "4 300 4" "6 120 8" "2 500 3" "8 40 4" "3 400 1" "8 16 1" "8 30 1" "8 30 8" "disjoint 9 9 5 1" \
             "disjoint 9 9 5 8" "disjoint 4 16 8 3"; do
    echo "-- $cfg"
    timeout 600 "$tmp/flooder_san" $cfg 2>&1 | grep -i "cells,\|sanitizer\|ERROR\|WARNING" | cut -c1-200
    echo "   exit ${PIPESTATUS[0]}"
  done
  echo "-- host_pool_main"
  timeout 600 "$tmp/pool_san" 2>&1 | grep -i "all ok\|FAILED\|sanitizer\|ERROR\|WARNING" | cut -c1-200
  echo "   exit ${PIPESTATUS[0]}"
done
