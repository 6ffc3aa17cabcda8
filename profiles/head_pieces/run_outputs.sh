#!/bin/bash
# run_outputs.sh PARENT_LIB OUT_DIR — check (d) of README.md: every group of dump_outputs.py under the parent's library twice (it must
# reproduce itself) and under the tree's own library, each run a fresh process under its own time limit, in that group's environment;
# then the byte comparison.  The first failure of a run ends the job; a comparison that differs is reported and the job goes on.
parent=$1; out=$2
here=$(cd "$(dirname "$0")" && pwd)
mkdir -p "$out"
run() {   # run TAG GROUP [ENV=VALUE ...]
    tag=$1; group=$2; shift 2
    env "$@" GATV2_LIB="$parent" timeout -k 10 240 python3 "$here/dump_outputs.py" "$group" "$out/$tag.parent1.npz" || exit 1
    env "$@" GATV2_LIB="$parent" timeout -k 10 240 python3 "$here/dump_outputs.py" "$group" "$out/$tag.parent2.npz" || exit 1
    env "$@" timeout -k 10 240 python3 "$here/dump_outputs.py" "$group" "$out/$tag.branch.npz" || exit 1
    python3 "$here/compare_outputs.py" "$tag parent / parent" "$out/$tag.parent1.npz" "$out/$tag.parent2.npz"
    python3 "$here/compare_outputs.py" "$tag parent / branch" "$out/$tag.parent1.npz" "$out/$tag.branch.npz"
}
run head head
run child_fuse "child:GAT_FUSE_LAST=1" GAT_FUSE_LAST=1
run child_nodes256 "child:GAT_HEAD_NODES=256" GAT_HEAD_NODES=256
run child_fuse_nodes256 "child:GAT_FUSE_LAST=1 GAT_HEAD_NODES=256" GAT_FUSE_LAST=1 GAT_HEAD_NODES=256
run loss loss
run loss_any loss GAT_LOSS_BLOCKED=0
run kinds kinds
echo "run_outputs: done"
