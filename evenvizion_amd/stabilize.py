"""Command-line driver of the stabilised view, with the arguments of the reference's
evenvizion/examples/compare_evenvizion_with_original_video.py plus --mode, --placement and --scale:

    python -m evenvizion_amd.stabilize --path_to_homography_dict run1/video/dict_with_homography_matrix.json \
           --path_to_video video.mp4 --experiment_name run1 --mode history --placement warp

writes  <cwd>/<experiment_name>/<video stem>/visualize_camera_stabilization/NNNNNN.ppm : per frame (one file for --mode
mosaic) the canvas of the fixed coordinate system as binary P6, produced on the MI355X by evenvizion_amd.stabilization.
Only the geometry of the reference's pictures is reproduced: no "Original" / "EvenVizion" text, no frame or canvas border,
no dimming of earlier frames and no side-by-side original are drawn, and the files are PPM, not PNG.
"""
import argparse
import os


def main(argv=None):
    ap = argparse.ArgumentParser(
        description="Stabilised view on MI355X (argument surface of compare_evenvizion_with_original_video.py).  Writes the "
                    "fixed-plane canvas per frame as binary PPM; draws no text, no border and no dimming of earlier frames.")
    ap.add_argument("--path_to_homography_dict", help="path to homography dict",
                    default="test_video_processing/test_video/dict_with_homography_matrix.json")
    ap.add_argument("--path_to_video", default="test_video/test_video.mp4")
    ap.add_argument("--experiment_name", help="folder to save experiment result", default="test_video_processing")
    ap.add_argument("--mode", choices=("history", "each", "mosaic"), default="history",
                    help="history: the canvas after every frame (the reference's picture); each: every frame alone; "
                         "mosaic: one canvas of all frames")
    ap.add_argument("--placement", choices=("warp", "translate"), default="translate",
                    help="translate: the reference's paste of the resized frame; warp: the projective warp of the full-size frame")
    ap.add_argument("--scale", type=float, default=1.0, help="warp only: canvas pixels per fixed-plane unit")
    args = ap.parse_args(argv)
    from .component import open_capture
    from .processing.utils import read_homography_dict, superposition_dict
    from .stabilization import stabilized_frames, write_ppm
    cap, _, stem = open_capture(args.path_to_video)
    save_folder = os.path.join(os.getcwd(), args.experiment_name, stem, "visualize_camera_stabilization")
    os.makedirs(save_folder, exist_ok=True)
    homography_dict, resize_info = read_homography_dict(args.path_to_homography_dict)
    sup = superposition_dict(homography_dict)
    for frame_no, picture in stabilized_frames(cap, sup, resize_info, mode=args.mode, placement=args.placement,
                                               scale=args.scale):
        write_ppm(os.path.join(save_folder, "%06d.ppm" % frame_no), picture)
    return save_folder


if __name__ == "__main__":
    main()
