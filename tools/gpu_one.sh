#!/bin/bash
# run one pytest selection on the GPU box:  tools/gpu_one.sh "<pytest args>"
mkdir -p out/one
timeout 1200 python -m pytest $1 -m gpu -x -q > out/one/tests.log 2>&1
echo "tests rc=$?" >> out/one/tests.log
tail -40 out/one/tests.log
