#!/bin/bash
# usage: build_reduce_lab.sh   ->  tools/native/reduce_lab, linked against semanticlens_amd/lib/libsemanticlens_hip.so (build that first)
set -e
cd "$(dirname "$0")"
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -I../../include "$@" reduce_lab.hip -o reduce_lab \
  -L../../semanticlens_amd/lib -lsemanticlens_hip '-Wl,-rpath,$ORIGIN/../../semanticlens_amd/lib'
ls -la reduce_lab
