"""Command-line driver with the argument surface and the non-visual outputs of the reference's example script
(evenvizion/examples/evenvizion_component.py:101-140), running the hot path on the MI355X.

    python -m evenvizion_amd.component --path_to_video frames.npy --experiment_name run1 --resize_width 400 \
           --path_to_original_coordinate original_coordinates.json

writes, like the reference, under  <cwd>/<experiment_name>/<video stem>/ :
    dict_with_homography_matrix.json   {frame_no: {"H": 3x3}, ..., "resize_info": {"h","w"}}   (:139-140)
    metrics_file.txt                   "Maximum movement during the entire video: <f64>"        (:62-65)
and, as a data file instead of the reference's rendered comparison video (:69-97),
    fixed_coordinates.json             from_original_to_fix(original coordinates) per frame;
with --heatmap_pictures 1 (extension, default off) also the reference's heat-map pictures without their drawing,
    heatmap_visualization/img%06d.ppm  the colours of heatmap_frame_processing over the resized frame, one per frame
                                       (heatmap.heatmap_frames: evh_heatmap_render; no grid lines, arrows or text; PPM, not PNG).
with --matching_pictures 1 (extension, default off) also the reference's matching pictures (:113-137, video_processing.py:76-81),
    matching_visualization/matching_vis_{i}.png   the resized frames i-1 | i and one green line per static match, for every
                                       pair whose matching succeeded (get_homography_dict(matching_sink=): evh_draw_matches,
                                       drawn in the same pass; --path_to_video only).

with --registration_report 1 (extension, default off) also a score for every matrix,
    registration_report.json           per pair of consecutive frames the motion-compensated residual under the pair's matrix and
                                       without it (covered pixels, sums of |difference| and difference^2 in gray, PSNR), their means
                                       over the video (itf, itf_unregistered) and the frames in order of least gain
                                       (registration.registration_report: evh_pair_residual; inf is written as Infinity).
with --residual_pictures 1 (extension, default off) also the difference pictures behind those figures,
    registration_visualization/res%06d.ppm   |current frame - registered previous frame| in gray, in all three channels.
with --reject_moving 1 (extension, default off; --path_to_video and --features ORB only) also a second pass that drops the matches on moving objects,
    dict_with_homography_matrix_refined.json   the dictionary of moving.refine_homography_dict: the first pass's background plate
                                       (stabilization.background_plate over --plate_frames frames), then every chunk's match rows
                                       judged against it (evh_rows_moving_filter: --moving_threshold, --moving_radius,
                                       --moving_min_cover) before the final solve; the first dictionary stays as it is
    moving_rows.json                   {frame_no: {"rows", "moving", "rows_out"}} per pair
    registration_report_refined.json   with --registration_report 1: the refined dictionary scored like the first one.
with --anchor_mosaic 1 (extension, default off; --path_to_video only) also frame-to-mosaic registration,
    dict_with_homography_matrix_anchored.json   the dictionary of registration.anchored_homography_dict: every frame (or group of
                                       --anchor_group frames) aligned against the blended mosaic of the frames before it
                                       (evh_canvas_refine) and then painted into it; the first dictionary stays as it is
    anchor_report.json                 the registration report of both dictionaries, the two canvas-score sums and a row per frame.
with --global_align 1 (extension, default off; --path_to_video only) also the whole chain aligned at once,
    dict_with_homography_matrix_aligned.json    the dictionary of graph.aligned_homography_dict: consecutive frames and frames that see
                                       the same ground again (--graph_gap, --graph_partners, --graph_min_inliers) matched, the rows of all those pairs in
                                       one least-squares problem over every frame's matrix (evh_graph_normal), solved for
                                       --graph_model; the first dictionary stays as it is
    graph_report.json                  the edges tried and kept, the loop edges per frame, the cost before and after, the steps
                                       and the registration report of both dictionaries.
with --recover_tracking 1 (extension, default off; --path_to_video and --features ORB only) also a second pass for the pairs whose matching failed,
    dict_with_homography_matrix_recovered.json  the dictionary of tracking.recover_homography_dict: such a pair's rows come from points
                                       followed on the pixels (evh_track_seeds, evh_track_points: --track_levels, --track_radius,
                                       --track_cell, --track_fb, --track_min_eig); the first dictionary stays as it is.  Where the
                                       first pass cannot finish (no matrix for the first pair) only these two files are written
    tracking_report.json               {frame_no: {"first_status", "seeds", "tracked", "flags", "final_status"}} per tracked pair.
--path_to_video takes what the reference's script takes for H.264 video in an MP4/MOV container: the file is opened by
evenvizion_amd.capture.VideoCapture (libevcap.so: this repository's own demultiplexer + H.264 decoder, standing in for
cv2.VideoCapture at evenvizion_component.py:132), e.g. the reference's own evenvizion/examples/test_video/test_video.mp4.
It also takes a .npy file (uint8 [F,h,w,3] BGR or [F,h,w] gray) or "synthetic:<frames>:<w>x<h>[:<seed>]".
--path_to_videos A B ... (extension) takes several of them and writes, per video, what the single form writes; the videos run
together through get_homography_dicts (several captures per GPU call), main() then returns the list of folders.
Differences, all deliberate: the matching pictures come under their own flag (--show_matching_visualization still has to stay
off: it refuses and names --matching_pictures) and the heat-map pictures only on request and without part_line's drawing; --resize_width is honoured (the reference script parses
it but never passes it on, so it always runs at 400 -- the default here).
"""
import argparse
import json
import os

import numpy as np


def _bool(v):
    if isinstance(v, bool):
        return v
    return str(v).strip().lower() not in ("0", "false", "no", "none", "")


VIDEO_SUFFIXES = (".mp4", ".mov", ".m4v")


def open_capture(spec):
    """-> (capture with .read() like cv2.VideoCapture, [h, w] of its frames, stem used for the output folder)"""
    from .synthetic import SyntheticCapture
    if spec.lower().endswith(VIDEO_SUFFIXES):
        from . import capture
        cap = capture.VideoCapture(spec)                                  # evenvizion_component.py:132
        if not cap.isOpened():
            raise ValueError("cannot open video %s: %s" % (spec, cap.open_error))
        return cap, [cap.height, cap.width], os.path.split(spec)[-1].split(".")[0]
    frames, stem = load_frames(spec)
    return SyntheticCapture(frames), [int(frames[0].shape[0]), int(frames[0].shape[1])], stem


def load_frames(spec):
    """-> (list of uint8 frames, stem used for the output folder)"""
    from . import synthetic as S
    if spec.startswith("synthetic:"):
        parts = spec.split(":")
        n = int(parts[1])
        w, h = (int(v) for v in parts[2].lower().split("x"))
        seed = int(parts[3]) if len(parts) > 3 else 1
        gray, _ = S.make_stream(seed, n, w, h)
        return list(S.gray_to_bgr(gray)), "synthetic_%d_%dx%d_%d" % (n, w, h, seed)
    arr = np.load(spec, allow_pickle=False)
    if arr.dtype != np.uint8 or arr.ndim not in (3, 4):
        raise ValueError("expected a uint8 array [F,h,w] or [F,h,w,3] in %s" % spec)
    return list(arr), os.path.split(spec)[-1].split(".")[0]


def _int_in(lo, hi):
    def parse(text):
        try:
            v = int(text)
        except ValueError:
            raise argparse.ArgumentTypeError("%r is not an integer" % text)
        if not lo <= v <= hi:
            raise argparse.ArgumentTypeError("%d is outside %d..%d" % (v, lo, hi))
        return v
    return parse


def parser():
    ap = argparse.ArgumentParser(description="EvenVizion hot path on MI355X (argument surface of evenvizion_component.py)")
    ap.add_argument("--path_to_video", type=str, default="synthetic:16:400x224:1")
    ap.add_argument("--path_to_videos", type=str, nargs="+", default=None,
                    help="several videos at once (extension): per video the outputs of --path_to_video, computed together")
    ap.add_argument("--max_streams", type=int, default=None, help="--path_to_videos: videos live in one GPU call")
    ap.add_argument("--decode_threads", type=int, default=None, help="--path_to_videos: host threads reading frames")
    ap.add_argument("--experiment_name", type=str, default="test_video_processing")
    ap.add_argument("--resize_width", type=int, default=400, help="width to resize frames to")
    ap.add_argument("--path_to_original_coordinate", default=None, help="path to json with original coordinates")
    ap.add_argument("--none_H_processing", default=True, help="If True use H_prev as H, False - do nothing")
    ap.add_argument("--heatmap_visualization", default=True, help="write metrics_file.txt (pictures are not rendered)")
    ap.add_argument("--heatmap_pictures", default=False,
                    help="also write heatmap_visualization/img%%06d.ppm: the heat-map colours over every resized frame, "
                         "without grid, arrows or text (extension; the video is read a second time)")
    ap.add_argument("--registration_report", default=False,
                    help="also write registration_report.json: the motion-compensated residual and PSNR of every pair of frames "
                         "under its matrix (extension; the video is read a second time)")
    ap.add_argument("--residual_pictures", default=False,
                    help="also write registration_visualization/res%%06d.ppm: the registered difference of every pair in gray "
                         "(extension; the video is read a second time)")
    ap.add_argument("--show_matching_visualization", default=False, help="not taken: use --matching_pictures")
    ap.add_argument("--matching_pictures", default=False,
                    help="also write matching_visualization/matching_vis_{i}.png: the resized frames i-1 | i with a green line "
                         "per static match (extension; drawn on the device in the same pass; --path_to_video only)")
    ap.add_argument("--features", type=str, default="SURF,SIFT,ORB",
                    help="feature types in FrameProcessing order (extension; the reference hard-wires SURF,SIFT,ORB)")
    ap.add_argument("--ingest", type=str, default="bgr", choices=("auto", "bgr", "yuv420"),
                    help="how frames reach the GPU: BGR frames (default), the decoder's 4:2:0 planes when the capture offers them "
                         "(auto), or planes only (extension; results do not depend on it)")
    ap.add_argument("--reject_moving", type=int, choices=(0, 1), default=0,
                    help="1: a second pass that drops the matches on moving objects (extension; --path_to_video and --features ORB only): the "
                         "background plate of the first pass, then moving.refine_homography_dict; writes "
                         "dict_with_homography_matrix_refined.json and moving_rows.json beside the first dictionary, which "
                         "stays as it is (the video is read twice more)")
    ap.add_argument("--moving_threshold", type=_int_in(0, 255), default=16,
                    help="--reject_moving: gray levels a point's surroundings must differ from the plate by")
    ap.add_argument("--moving_radius", type=_int_in(0, 7), default=1,
                    help="--reject_moving: the window around a point is (2*radius + 1)^2 canvas pixels")
    ap.add_argument("--moving_min_cover", type=_int_in(1, 255), default=2,
                    help="--reject_moving: frames of the plate that must cover a canvas pixel for it to be judged")
    ap.add_argument("--plate_frames", type=_int_in(1, 255), default=64, help="--reject_moving: frames the plate is taken over")
    ap.add_argument("--refine_direct", type=int, choices=(0, 1), default=0,
                    help="1: direct alignment of every pair on the pixels, starting from the dictionary's matrices (extension; "
                         "--path_to_video only): registration.refined_homography_dict; writes "
                         "dict_with_homography_matrix_direct.json and direct_report.json beside the first dictionary, which "
                         "stays as it is (the video is read three times more)")
    ap.add_argument("--refine_levels", type=_int_in(1, 4), default=1, help="--refine_direct: pyramid levels, coarse to fine")
    ap.add_argument("--refine_iters", type=_int_in(0, 64), default=8, help="--refine_direct: steps tried per level")
    ap.add_argument("--recover_tracking", type=int, choices=(0, 1), default=0,
                    help="1: a second pass that gives the pairs whose matching failed rows from points followed on the pixels "
                         "(extension; --path_to_video and --features ORB only): tracking.recover_homography_dict; writes "
                         "dict_with_homography_matrix_recovered.json and tracking_report.json beside the first dictionary, which "
                         "stays as it is (the video is read once more)")
    ap.add_argument("--track_levels", type=_int_in(1, 4), default=3, help="--recover_tracking: pyramid levels")
    ap.add_argument("--track_radius", type=_int_in(1, 10), default=7, help="--recover_tracking: the window is (2*radius + 1)^2 pixels")
    ap.add_argument("--track_cell", type=_int_in(8, 64), default=16, help="--recover_tracking: one seed per cell of this many pixels")
    ap.add_argument("--track_fb", type=float, default=0.5,
                    help="--recover_tracking: pixels a point may miss its start by when followed back; negative: no backward pass")
    ap.add_argument("--track_min_eig", type=float, default=None,
                    help="--recover_tracking: the smaller eigenvalue of the mean structure tensor a seed and a window must reach "
                         "(default: tracking.MIN_EIG)")
    ap.add_argument("--anchor_mosaic", type=int, choices=(0, 1), default=0,
                    help="1: frame-to-mosaic registration, every frame aligned against the blended picture of the frames before it "
                         "(extension; --path_to_video only): registration.anchored_homography_dict; writes "
                         "dict_with_homography_matrix_anchored.json and anchor_report.json beside the first dictionary, which "
                         "stays as it is (the video is read three times more)")
    ap.add_argument("--anchor_group", type=_int_in(1, 65535), default=1,
                    help="--anchor_mosaic: frames aligned and painted together (1: strictly frame by frame)")
    ap.add_argument("--global_align", type=int, choices=(0, 1), default=0,
                    help="1: the whole chain aligned at once (extension; --path_to_video only): graph.aligned_homography_dict; "
                         "writes dict_with_homography_matrix_aligned.json and graph_report.json beside the first dictionary, "
                         "which stays as it is (the video is read three times more)")
    ap.add_argument("--graph_model", type=str, default="homography", choices=("translation", "similarity", "affine", "homography"),
                    help="--global_align: the correction every frame's matrix may take")
    ap.add_argument("--graph_partners", type=_int_in(0, 64), default=4, help="--global_align: loop edges per frame at the most")
    ap.add_argument("--graph_min_inliers", type=_int_in(1, 65535), default=20,
                    help="--global_align: rows of a pair that must lie within 3 px of the pair's own matrix for its edge to be kept; "
                         "a consecutive pair below it breaks the chain and the alignment refuses, naming the pair")
    ap.add_argument("--graph_gap", type=_int_in(1, 65535), default=8,
                    help="--global_align: frames a loop partner lies back at the least, and two partners of a frame apart")
    return ap


def main(argv=None):
    args = parser().parse_args(argv)
    if _bool(args.show_matching_visualization):
        raise NotImplementedError("--show_matching_visualization is not taken: leave it off and ask for the matching pictures "
                                  "with --matching_pictures 1")

    from .processing.video_processing import get_homography_dict, get_homography_dicts
    features = [f for f in args.features.split(",") if f]
    if args.reject_moving and features != ["ORB"]:
        raise ValueError("--reject_moving takes --features ORB: the second pass is built on the fused ORB path only")
    if args.recover_tracking and features != ["ORB"]:
        raise ValueError("--recover_tracking takes --features ORB: the second pass is built on the fused ORB path only")
    if args.path_to_videos:
        if args.recover_tracking:
            raise ValueError("--recover_tracking takes one video (--path_to_video)")
        if _bool(args.matching_pictures):
            raise ValueError("--matching_pictures takes one video (--path_to_video)")
        if args.reject_moving:
            raise ValueError("--reject_moving takes one video (--path_to_video)")
        if args.refine_direct:
            raise ValueError("--refine_direct takes one video (--path_to_video)")
        if args.anchor_mosaic:
            raise ValueError("--anchor_mosaic takes one video (--path_to_video)")
        if args.global_align:
            raise ValueError("--global_align takes one video (--path_to_video)")
        opened = [open_capture(spec) for spec in args.path_to_videos]
        kw = {k: v for k, v in (("max_streams", args.max_streams), ("decode_threads", args.decode_threads)) if v is not None}
        results = get_homography_dicts([cap for cap, _, _ in opened], resize_width=args.resize_width,
                                       none_H_processing=_bool(args.none_H_processing), features_type_list=features,
                                       ingest=args.ingest, **kw)
        folders = []
        for n, (result, (_, original_shape, stem)) in enumerate(zip(results, opened)):
            if [s for _, _, s in opened].count(stem) > 1:
                stem = "%s_%d" % (stem, n)               # two videos of one name: one folder each
            folders.append(write_outputs(args, result, original_shape, stem, args.path_to_videos[n]))
        return folders
    cap, original_shape, stem = open_capture(args.path_to_video)
    sink = None
    if _bool(args.matching_pictures):
        from .matching_pictures import write_png
        pictures = os.path.join(output_folder(args, stem), "matching_visualization")      # evenvizion_component.py:134-137
        os.makedirs(pictures, exist_ok=True)

        def sink(frame_no, picture):
            write_png(os.path.join(pictures, "matching_vis_{}.png".format(frame_no)), picture)
    try:
        result = get_homography_dict(cap, resize_width=args.resize_width, matching_path=None,
                                     none_H_processing=_bool(args.none_H_processing),
                                     features_type_list=features, ingest=args.ingest, matching_sink=sink)
    except AttributeError as error:         # the reference's end of a video whose first pair has no matrix, and nothing else
        if not args.recover_tracking or "no homography for frame" not in str(error):
            raise
        from .processing.video_processing import resized_shape
        w, h = resized_shape(original_shape, args.resize_width)
        save_folder = output_folder(args, stem)
        os.makedirs(save_folder, exist_ok=True)
        write_recovered(args, save_folder, {"resize_info": {"h": h, "w": w}})
        return save_folder
    save_folder = write_outputs(args, result, original_shape, stem, args.path_to_video)
    if args.recover_tracking:
        write_recovered(args, save_folder)
    if args.reject_moving:
        write_refined(args, save_folder, features)
    if args.refine_direct:
        write_direct(args, save_folder)
    if args.anchor_mosaic:
        write_anchored(args, save_folder)
    if args.global_align:
        write_aligned(args, save_folder)
    return save_folder


def write_recovered(args, save_folder, first_pass=None):
    """--recover_tracking 1: the pairs the first pass lost solved from tracked points, the recovered dictionary and its report beside
    the first pass's files, which are left as they are.  first_pass: None = the dictionary in save_folder."""
    from .processing.utils import read_homography_dict
    from . import tracking
    if first_pass is None:
        matrices, resize_info = read_homography_dict(os.path.join(save_folder, "dict_with_homography_matrix.json"))
        first_pass = dict(matrices, resize_info=resize_info)
    recovered, report = tracking.recover_homography_dict(
        open_capture(args.path_to_video)[0], first_pass, levels=args.track_levels, radius=args.track_radius, cell=args.track_cell,
        fb_max=args.track_fb if args.track_fb >= 0 else None,
        min_eig=tracking.MIN_EIG if args.track_min_eig is None else args.track_min_eig, ingest=args.ingest,
        none_H_processing=_bool(args.none_H_processing))
    with open(os.path.join(save_folder, "dict_with_homography_matrix_recovered.json"), "w") as json_:
        json.dump(recovered, json_)
    with open(os.path.join(save_folder, "tracking_report.json"), "w") as json_:
        json.dump({str(k): v for k, v in report.items()}, json_)


def write_aligned(args, save_folder):
    """--global_align 1: the first pass's matrices aligned all at once, the aligned dictionary and its report beside the first
    pass's files, which are left as they are.  The capture is opened again for each pass."""
    from .processing.utils import read_homography_dict, superposition_dict
    from . import graph
    spec = args.path_to_video
    first_pass, resize_info = read_homography_dict(os.path.join(save_folder, "dict_with_homography_matrix.json"))
    got = graph.aligned_homography_dict(lambda: open_capture(spec)[0], superposition_dict(first_pass), resize_info, ingest=args.ingest,
                                        model=args.graph_model, max_partners=args.graph_partners, min_gap=args.graph_gap,
                                        min_inliers=args.graph_min_inliers)
    with open(os.path.join(save_folder, "dict_with_homography_matrix_aligned.json"), "w") as json_:
        json.dump(dict(got["homography"], resize_info=resize_info), json_)
    report = dict(got["report"])
    report["loop_edges"] = {str(k): v for k, v in report["loop_edges"].items()}
    report["loop_edges_kept"] = {str(k): v for k, v in report.get("loop_edges_kept", {}).items()}
    with open(os.path.join(save_folder, "graph_report.json"), "w") as json_:
        json.dump(report, json_)


def write_anchored(args, save_folder):
    """--anchor_mosaic 1: the first pass's matrices anchored on their own mosaic, the anchored dictionary and the score of both
    beside the first pass's files, which are left as they are.  The capture is opened again for each pass."""
    from .processing.utils import read_homography_dict, superposition_dict
    from . import registration
    spec = args.path_to_video
    first_pass, resize_info = read_homography_dict(os.path.join(save_folder, "dict_with_homography_matrix.json"))
    got = registration.anchored_homography_dict(lambda: open_capture(spec)[0], superposition_dict(first_pass), resize_info,
                                                group=args.anchor_group, ingest=args.ingest)
    with open(os.path.join(save_folder, "dict_with_homography_matrix_anchored.json"), "w") as json_:
        json.dump(dict(got["homography"], resize_info=resize_info), json_)
    with open(os.path.join(save_folder, "anchor_report.json"), "w") as json_:
        json.dump({"before": got["report_before"], "after": got["report_after"],
                   "canvas_score_before": got["canvas_score_before"], "canvas_score_after": got["canvas_score_after"],
                   "info": {str(k): v for k, v in got["info"].items()}}, json_)


def write_direct(args, save_folder):
    """--refine_direct 1: the first pass's matrices refined on the pixels, the refined dictionary and the score of both beside the
    first pass's files, which are left as they are.  The capture is opened again for each pass."""
    from .processing.utils import read_homography_dict, superposition_dict
    from . import registration
    spec = args.path_to_video
    first_pass, resize_info = read_homography_dict(os.path.join(save_folder, "dict_with_homography_matrix.json"))
    got = registration.refined_homography_dict(lambda: open_capture(spec)[0], superposition_dict(first_pass), resize_info,
                                               iters=args.refine_iters, levels=args.refine_levels, ingest=args.ingest)
    with open(os.path.join(save_folder, "dict_with_homography_matrix_direct.json"), "w") as json_:
        json.dump(dict(got["homography"], resize_info=resize_info), json_)
    with open(os.path.join(save_folder, "direct_report.json"), "w") as json_:
        json.dump({"before": got["report_before"], "after": got["report_after"],
                   "info": {str(k): v for k, v in got["info"].items()}}, json_)


def write_refined(args, save_folder, features):
    """--reject_moving 1: the background plate of the first pass's dictionary, the second pass against it, and its files beside
    the first pass's, which are left as they are.  The capture is opened again for each pass."""
    from .processing.utils import read_homography_dict, superposition_dict
    from .stabilization import background_plate
    from .moving import refine_homography_dict
    spec = args.path_to_video
    first_pass, resize_info = read_homography_dict(os.path.join(save_folder, "dict_with_homography_matrix.json"))
    plate = background_plate(open_capture(spec)[0], superposition_dict(first_pass), resize_info, placement="warp",
                             max_frames=args.plate_frames, min_cover=args.moving_min_cover, ingest=args.ingest)
    refined, stats = refine_homography_dict(open_capture(spec)[0], dict(first_pass, resize_info=resize_info), plate,
                                            placement="warp", threshold=args.moving_threshold, min_cover=args.moving_min_cover,
                                            radius=args.moving_radius, features_type_list=features, ingest=args.ingest,
                                            none_H_processing=_bool(args.none_H_processing))
    path = os.path.join(save_folder, "dict_with_homography_matrix_refined.json")
    with open(path, "w") as json_:
        json.dump(refined, json_)
    with open(os.path.join(save_folder, "moving_rows.json"), "w") as json_:
        json.dump({str(k): {"rows": v[0], "moving": v[1], "rows_out": v[2]} for k, v in stats.items()}, json_)
    if _bool(args.registration_report):
        from . import registration
        matrices, resize_info = read_homography_dict(path)
        report = registration.registration_report(open_capture(spec)[0], superposition_dict(matrices), resize_info, ingest=args.ingest)
        with open(os.path.join(save_folder, "registration_report_refined.json"), "w") as json_:
            json.dump(report, json_)


def output_folder(args, stem):
    return os.path.join(os.getcwd(), args.experiment_name, stem)


def write_outputs(args, result, original_shape, stem, spec=None):
    """One video's files under <cwd>/<experiment_name>/<stem>/ (evenvizion_component.py:62-65,139-140) -> the folder.
    spec: what the video was opened from, to read it again for --heatmap_pictures, --registration_report and --residual_pictures."""
    from .processing.utils import read_homography_dict, superposition_dict, read_json_with_coordinates, \
        are_infinity_coordinates
    from .processing.fixed_coordinate_system import from_original_to_fix
    from . import heatmap

    save_folder = output_folder(args, stem)
    os.makedirs(save_folder, exist_ok=True)
    path_to_homography_dict = os.path.join(save_folder, "dict_with_homography_matrix.json")
    with open(path_to_homography_dict, "w") as json_:
        json.dump(result, json_)

    homography_matrices, resize_info = read_homography_dict(path_to_homography_dict)
    reformat = superposition_dict(homography_matrices)
    if _bool(args.heatmap_visualization):
        keys, per_frame = heatmap.frame_maxima(reformat, resize_info)
        max_movement = per_frame[:-1] if len(per_frame) > 1 else per_frame       # the reference never appends the last frame
        with open(os.path.join(save_folder, "metrics_file.txt"), "w") as txt_:
            txt_.write("Maximum movement during the entire video: {}".format(np.max(max_movement)))
            if are_infinity_coordinates(max_movement):
                txt_.write("There are some frames with undefined coordinates")
    if _bool(args.heatmap_pictures):
        from .stabilization import write_ppm
        pictures = os.path.join(save_folder, "heatmap_visualization")
        os.makedirs(pictures, exist_ok=True)
        cap = open_capture(spec)[0]                              # visualize_heatmap opens the video again too (:52)
        for frame_no, picture in heatmap.heatmap_frames(cap, reformat, resize_info, ingest=args.ingest):
            write_ppm(os.path.join(pictures, "img%06d.ppm" % int(frame_no)), picture)
    if _bool(args.registration_report):
        from . import registration
        report = registration.registration_report(open_capture(spec)[0], reformat, resize_info, ingest=args.ingest)
        with open(os.path.join(save_folder, "registration_report.json"), "w") as json_:
            json.dump(report, json_)
    if _bool(args.residual_pictures):
        from . import registration
        from .stabilization import write_ppm
        pictures = os.path.join(save_folder, "registration_visualization")
        os.makedirs(pictures, exist_ok=True)
        for frame_no, picture in registration.residual_frames(open_capture(spec)[0], reformat, resize_info, ingest=args.ingest):
            write_ppm(os.path.join(pictures, "res%06d.ppm" % int(frame_no)), np.repeat(picture[:, :, None], 3, axis=2))
    if args.path_to_original_coordinate:
        original_coordinates = read_json_with_coordinates(args.path_to_original_coordinate)
        fixed = from_original_to_fix(original_coordinates, reformat, original_shape, [resize_info["h"], resize_info["w"]])
        with open(os.path.join(save_folder, "fixed_coordinates.json"), "w") as json_:
            json.dump(fixed, json_)
    return save_folder


if __name__ == "__main__":
    print(main())
