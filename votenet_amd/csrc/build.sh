#!/usr/bin/env bash
# Builds votenet_amd/lib/libvotenet_hip.so for gfx950 (MI355X).  hipcc cross-compiles without a GPU.
# -ffp-contract=off: distance / interpolation expressions must be evaluated un-fused, left to
# right, exactly as the reference writes them (bit-exact FPS picks and ball-query decisions).
set -euo pipefail
HERE="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
OUT="$HERE/../lib"
mkdir -p "$OUT" "$HERE/obj"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -fvisibility=hidden -ffp-contract=off -Wall -Wno-unused-function"
# An object is stale when its source, this script (it carries the flags) or ANY header of the project is newer: no list to keep by hand.
stale() { # object, source
  local dep
  [ -f "$1" ] || return 0
  for dep in "$2" "${BASH_SOURCE[0]}" "$HERE"/*.h "$HERE"/*/*.h "$HERE"/../../include/*.h; do
    [ "$dep" -nt "$1" ] && return 0
  done
  return 1
}
pids=()
for src in "$HERE"/*.hip; do
  obj="$HERE/obj/$(basename "${src%.hip}").o"
  if stale "$obj" "$src"; then
    extra=""
    # fps.hip: no NaN can occur (distances of finite points); dropping NaN canonicalisation shortens the
    # serial per-round instruction chain.  Infinities (empty bucket boxes) are still honoured.
    [ "$(basename "$src")" = "fps.hip" ] && extra="-fno-honor-nans"
    # half.hip, loss.hip: no SLP vectorisation -- packing two scalar multiply-adds that share a multiplier held in the odd register of a
    # pair gives v_pk_*_f32 with op_sel[1] = 1, which returns wrong low halves beside another kernel's MFMA wavefronts
    # (tools/check_isa_hazards.py, run below on the linked library)
    case "$(basename "$src")" in half.hip|loss.hip) extra="-fno-slp-vectorize" ;; esac
    $HIPCC $FLAGS $extra -c "$src" -o "$obj" &
    pids+=($!)
  fi
done
for p in "${pids[@]:-}"; do [ -n "$p" ] && wait "$p"; done
# Link under a temporary name, run the ISA-hazard gate on THAT, and only then move it into place: a library that fails the gate never
# becomes the one later imports load.  exports.map: only the votenet_* C ABI and the reference's eight launcher names are visible.
TMP="$OUT/.libvotenet_hip.so.tmp.$$"
trap 'rm -f "$OUT"/.lib*.so.tmp.$$' EXIT # whatever temporary this run has made, the side libraries' below included
$HIPCC --offload-arch=gfx950 -shared -fPIC -Wl,--version-script="$HERE/exports.map" "$HERE"/obj/*.o -o "$TMP"
python3 "$HERE/../../tools/check_isa_hazards.py" "$TMP"
mv -f "$TMP" "$OUT/libvotenet_hip.so"
echo "built $OUT/libvotenet_hip.so"
# The side libraries: what must stay out of the drop-in library's export list (the reference's ops) ships as a library of its own, with
# its own header under include/ and its own exports.map.  Same flags, same gate.  One row each: directory, source, library, extra flags.
SIDE_LIBS=(
  # the training summaries.  -fno-slp-vectorize as loss.hip, whose assignment loop (nearest_box.h) it shares
  "monitors monitors.hip       monitors -fno-slp-vectorize"
  # the guarded optimizer step.  sumsq.h is the text of votenet_clip_adam's partial sums, so both libraries form the same bits
  "guard    step_guard.hip     guard    -fno-slp-vectorize"
  # the input step of a network with point features.  augment_points.h is the text of votenet_subsample_augment's points
  "features point_features.hip features"
  # class-wise 3D NMS, per-class detections and their matching.  iou3d.h is the text of votenet_iou3d_matrix's overlaps
  "detect   detections.hip     detect"
  # the points inside each predicted box and the empty-box gate.  No contraction: tests/box_points_ref.py restates the rule operation
  # for operation; -fno-slp-vectorize as loss.hip: the point slots' dot products pack into the v_pk_*_f32 forms the gate refuses
  "boxpts   box_points.hip     boxpts   -fno-slp-vectorize"
  # the axis-aligned overlaps of the paper's NMS (tests/aabb_nms_ref.py restates them).  -fno-slp-vectorize as box_points.hip: the three
  # axes' products would pack likewise.  detect/det_emit.h is the text of votenet_class_nms3d's rows, so both libraries write the same bytes
  "aabb     aabb_nms.hip       aabb     -fno-slp-vectorize"
  # the raw scan from the depth image.  No contraction: tests/depth_scan_ref.py restates the rule operation for operation in double
  "depth    depth_scan.hip     depth"
  # the paper's vote supervision, one launch behind the loss.  No contraction: tests/vote_supervision_ref.py restates the rule operation
  # for operation; -fno-slp-vectorize as box_points.hip: the seed slots' rotations would pack likewise
  "votesup  vote_supervision.hip votesup -fno-slp-vectorize"
  # the paper's objectness and centre supervision, one launch behind the loss.  No contraction: tests/proposal_supervision_ref.py restates
  # the rule operation for operation; -fno-slp-vectorize as loss.hip, whose assignment loop (nearest_box.h) it shares
  "propsup  proposal_supervision.hip propsup -fno-slp-vectorize"
  # the proposal module's clusters sampled on the votes, one launch.  No contraction: the picks and hits are fps.hip's and grouping.hip's,
  # decided by the same un-fused expressions (ball_threshold.h is the text of votenet_query_ball_point's threshold);
  # -fno-slp-vectorize as box_points.hip: the three axes' products would pack likewise
  "votesamp vote_sampling.hip  votesamp -fno-slp-vectorize"
  # ground-truth boxes from instance-labelled points.  No contraction, as everywhere: tests/instance_boxes_ref.py restates the rule and
  # every output is compared by bit pattern (the combinations are integer atomics; the only float arithmetic is the rows' in double)
  "instbox  instance_boxes.hip instbox"
  # vote supervision from instance labels, one launch behind the loss.  No contraction: tests/instance_votes_ref.py restates the rule
  # operation for operation; -fno-slp-vectorize as votesup, whose loss and cotangent these are: the three axes' differences would pack
  "instvote instance_votes.hip instvote -fno-slp-vectorize"
  # the vote features divided by their L2 norm, as the authors' VoteNet does: one launch each way in the place of a glue launch.  No
  # contraction: tests/unit_votes_ref.py restates the rule operation for operation and every output is compared by bit pattern;
  # -fno-slp-vectorize as loss.hip: a lane's neighbouring channels' sums, squares and quotients would pack into the forms the gate refuses
  "unitvote unit_votes.hip unitvote -fno-slp-vectorize"
)
side_lib() { # directory, source, library name, extra flags ...
  local dir="$HERE/$1" src="$HERE/$1/$2" lib="libvotenet_$3.so" obj="$HERE/$1/obj/$(basename "${2%.hip}").o" tmp
  shift 3
  mkdir -p "$dir/obj"
  if stale "$obj" "$src"; then $HIPCC $FLAGS "$@" -c "$src" -o "$obj"; fi
  tmp="$OUT/.$lib.tmp.$$"
  $HIPCC --offload-arch=gfx950 -shared -fPIC -Wl,--version-script="$dir/exports.map" "$obj" -o "$tmp"
  python3 "$HERE/../../tools/check_isa_hazards.py" "$tmp"
  mv -f "$tmp" "$OUT/$lib"
  echo "built $OUT/$lib"
}
for row in "${SIDE_LIBS[@]}"; do side_lib $row; done
