#!/usr/bin/env python3
"""Entry point with the reference's command line (/root/reference main.py:29-56): the modes that lie on
the hot path run on the HIP engine; dataset preprocessing is outside this build's scope and says so.

    python main.py --mode train_joint --config config/config.yaml
    python main.py --mode train_classifier                         # fog-intensity classifier: train, then evaluate
    python main.py --mode train_joint --resume                     # continue from the latest checkpoint
    torchrun --nproc-per-node 8 main.py --mode train_joint        # data-parallel over RCCL
    python main.py --mode demo --input DIR --output OUT --panels   # dehaze image files at their own size
    python main.py --mode demo --input HAZY --target CLEAR         # ... and score them: PSNR, SSIM, CIEDE2000 per file
    python main.py --mode demo --input HAZY --target CLEAR --ms-ssim   # ... plus Gaussian-window SSIM and MS-SSIM
    python main.py --mode demo --input DIR --detect                # ... detect on hazy and dehazed, boxes drawn on the device
    python main.py --mode demo --input CLEAR --fit-niqe niqe.npz   # fit a NIQE model from clean files
    python main.py --mode demo --input DIR --niqe niqe.npz         # ... and score without ground truth: NIQE per file
    python main.py --mode synthesize --input CLEAR --depth DEPTH --output OUT   # render {low,medium,high}/{hazy,clear} pairs
    python main.py --mode synthesize --input CLEAR --nonuniform --chromatic     # ... under patchy, tinted haze

`--resume` is the reference's flag (main.py:50-51 parses it and never reads it); here it restores model, optimiser,
scheduler, epoch and best-PSNR from the latest checkpoint of the mode's checkpoint directory (or from the file given
as its optional value).  `--data_dir D` sets the dataset paths like the reference does (D/train, D/val, D/test); the drivers
read `<path>/<split>/{low,medium,high}/{hazy,clear}` (or `<path>/{low,medium,high}/...`) from there into a device-resident
cache, and only when no such folders exist do they say loudly that they train on synthetic frames.
"""
import argparse
import os
import random

import numpy as np
import torch
import yaml


def parse_args():
    p = argparse.ArgumentParser(description="Adaptive fog intensity dehazing framework (MI355X build)")
    p.add_argument("--config", type=str, default="config/config.yaml")
    p.add_argument("--mode", type=str, default="train_all",
                   choices=["preprocess", "train_classifier", "train_dehazing", "train_joint", "train_all", "evaluate", "demo",
                            "synthesize"])
    p.add_argument("--exp_name", type=str, default=None)
    p.add_argument("--data_dir", type=str, default=None)
    p.add_argument("--device", type=str, default=None)
    p.add_argument("--resume", nargs="?", const=True, default=None,
                   help="resume training from the latest checkpoint (or from the given checkpoint file)")
    p.add_argument("--seed", type=int, default=None)
    p.add_argument("--epochs", type=int, default=None, help="override the configured number of epochs")
    p.add_argument("--input", type=str, default=None,
                   help="--mode demo: an image file, or a directory of *.png / *.jpg / *.jpeg / *.bmp files, to dehaze")
    p.add_argument("--output", type=str, default="demo", help="--mode demo: where the dehazed images and demo_results.json go")
    p.add_argument("--panels", action="store_true", help="--mode demo: also write <name>_panel.png, hazy | dehazed")
    p.add_argument("--target", type=str, default=None,
                   help="--mode demo --input ...: the ground truth, a directory matched to the inputs by base name, or one "
                        "file; scores every dehazed file (PSNR, SSIM, CIEDE2000) and writes demo_scores.json")
    p.add_argument("--self-ensemble", dest="self_ensemble", choices=["flip", "d8"], default=None,
                   help="--mode demo --input ...: average the output over the 4 flips (flip) or all 8 flips and rotations (d8) "
                        "of the input; overrides demo.self_ensemble of the config")
    p.add_argument("--exif", action="store_true",
                   help="--mode demo --input ...: turn every file (and every --target file) upright by its EXIF orientation "
                        "tag first; same as demo.exif_orientation: true in the config")
    p.add_argument("--ms-ssim", dest="ms_ssim", action="store_true",
                   help="--mode demo --input ... --target ...: also score the 11x11 Gaussian-window SSIM per colour channel and "
                        "the five-level MS-SSIM of the published tables; same as demo.ms_ssim: true in the config")
    p.add_argument("--detect", action="store_true",
                   help="--mode demo --input ...: run the detector on every hazy input and dehazed output, record and compare "
                        "the detections, and write <name>_detect.png (both panes annotated) and demo_detections.json; same as "
                        "demo.detect: true in the config")
    p.add_argument("--detect-threshold", dest="detect_threshold", type=float, default=None,
                   help="--detect: keep detections scoring above this (0..1; demo.detect_threshold, 0.5)")
    p.add_argument("--niqe", type=str, default=None, metavar="MODEL.npz",
                   help="--mode demo --input ...: score every dehazed file and every input with the no-reference NIQE against "
                        "this model (written by --fit-niqe); needs no --target; same as demo.niqe_model in the config")
    p.add_argument("--brisque-model", dest="brisque_model", type=str, default=None, metavar="FILE",
                   help="--mode demo --input ...: score with BRISQUE through this libsvm epsilon-SVR model file (not shipped); "
                        "same as demo.brisque_model in the config")
    p.add_argument("--brisque-range", dest="brisque_range", type=str, default=None, metavar="FILE",
                   help="--brisque-model: the svm-scale range file of its features (demo.brisque_range)")
    p.add_argument("--fit-niqe", dest="fit_niqe", type=str, default=None, metavar="OUT.npz",
                   help="--mode demo --input CLEAR_DIR: fit the NIQE model from these clean image files, write it and exit")
    p.add_argument("--depth", type=str, default=None, metavar="DEPTH_DIR",
                   help="--mode synthesize --input CLEAR_DIR: the directory of depth maps, <stem>.png (8-bit or 16-bit grey) per "
                        "clear file; without it the reference's radial depth map is used")
    p.add_argument("--nonuniform", action="store_true",
                   help="--mode synthesize: patchy haze, the optical depth scaled per pixel by a multi-octave noise field; the "
                        "values come from dataset.synthetic_haze.nonuniform in the config, else the defaults")
    p.add_argument("--chromatic", action="store_true",
                   help="--mode synthesize: wavelength-dependent beta and a tinted airlight per channel; the values come from "
                        "dataset.synthetic_haze.chromatic in the config, else the defaults")
    return p.parse_args()


def seed_everything(seed):
    """utils/helpers.py:10-19."""
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    torch.cuda.manual_seed_all(seed)
    os.environ["PYTHONHASHSEED"] = str(seed)


def main():
    args = parse_args()
    if args.target and not (args.mode == "demo" and args.input):
        # refused before anything is built: there would be nothing to score
        raise SystemExit("--target needs --mode demo --input DIR_OR_FILE: it names the ground truth of the image files "
                         "given with --input.")
    if (args.self_ensemble or args.exif) and not (args.mode == "demo" and args.input):
        raise SystemExit("--self-ensemble and --exif need --mode demo --input DIR_OR_FILE: they are options of dehazing image "
                         "files.")
    if (args.detect or args.detect_threshold is not None) and not (args.mode == "demo" and args.input):
        raise SystemExit("--detect and --detect-threshold need --mode demo --input DIR_OR_FILE: they are options of dehazing "
                         "image files.")
    if args.ms_ssim and not args.target:
        raise SystemExit("--ms-ssim needs --mode demo --input DIR_OR_FILE --target DIR_OR_FILE: MS-SSIM is a score against "
                         "the ground truth.")
    if (args.niqe or args.brisque_model or args.brisque_range) and not (args.mode == "demo" and args.input):
        raise SystemExit("--niqe, --brisque-model and --brisque-range need --mode demo --input DIR_OR_FILE: they score the "
                         "image files given with --input.")
    if args.brisque_range and not args.brisque_model:
        raise SystemExit("--brisque-range needs --brisque-model: it is the range file of that model's features.")
    if args.depth and args.mode != "synthesize":
        raise SystemExit("--depth needs --mode synthesize --input CLEAR_DIR: it names the depth maps of the clear files.")
    if (args.nonuniform or args.chromatic) and args.mode != "synthesize":
        raise SystemExit("--nonuniform / --chromatic need --mode synthesize (training reads dataset.synthetic_haze in the config).")
    if args.mode == "synthesize" and not args.input:
        raise SystemExit("--mode synthesize needs --input CLEAR_DIR (and takes --depth DEPTH_DIR, --output OUT, --seed S).")
    if args.fit_niqe:
        if not (args.mode == "demo" and args.input):
            raise SystemExit("--fit-niqe needs --mode demo --input CLEAR_DIR: the clean image files the model is fitted from.")
        others = [flag for flag, given in (("--target", args.target), ("--panels", args.panels),
                                           ("--self-ensemble", args.self_ensemble), ("--exif", args.exif),
                                           ("--ms-ssim", args.ms_ssim), ("--detect", args.detect),
                                           ("--detect-threshold", args.detect_threshold is not None), ("--niqe", args.niqe),
                                           ("--brisque-model", args.brisque_model), ("--brisque-range", args.brisque_range))
                  if given]
        if others:
            raise SystemExit(f"--fit-niqe fits a model and exits; it does not go with {', '.join(others)}.")
    with open(args.config) as f:
        config = yaml.safe_load(f)
    if args.data_dir:   # main.py:66-69
        config["dataset"]["train_path"] = os.path.join(args.data_dir, "train")
        config["dataset"]["val_path"] = os.path.join(args.data_dir, "val")
        config["dataset"]["test_path"] = os.path.join(args.data_dir, "test")
    if args.device:
        config["device"] = args.device
    if args.seed:
        config["seed"] = args.seed
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.mode == "train_classifier":
        # refused before any process group or device is touched
        if world > 1:
            raise SystemExit("--mode train_classifier runs in a single process: data-parallel classifier training is not "
                             "implemented.  Run it without torchrun (WORLD_SIZE=1).")
        if args.resume is not None:
            raise SystemExit("--resume is not supported for --mode train_classifier: the classifier stage always trains from "
                             "scratch (drop --resume).")
    if args.mode in ("demo", "synthesize") and args.input and world > 1:
        raise SystemExit(f"--mode {args.mode} runs in a single process.  Run it without torchrun (WORLD_SIZE=1).")
    if world > 1:
        import torch.distributed as dist
        local = int(os.environ.get("LOCAL_RANK", "0"))
        torch.cuda.set_device(local)
        config["device"] = f"cuda:{local}"
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        backend = os.environ.get("ADH_DIST_BACKEND", "nccl")   # nccl = RCCL over xGMI
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend)
    seed_everything(config["seed"])
    from adam_dehaze_amd import train as T

    def resume_for(stage):
        """Bare `--resume`: every stage discovers the latest checkpoint in its own directory.  `--resume <file>`: the file
        goes to the ONE stage that wrote it (a branch checkpoint loaded into another branch, or into the joint stage, used
        to fail with a KeyError deep in the loader); the other stages of a multi-stage mode start fresh."""
        if args.resume is None or args.resume is True:
            return args.resume
        if resume_owner != stage:
            print(f"--resume {args.resume}: a '{resume_owner}' checkpoint; stage '{stage}' does not resume from it")
            return None
        return args.resume
    # `--resume <file>`: resolve the stage that wrote the file ONCE (checkpoint_stage reads the file and compares key sets), and
    # refuse a mode that runs no such stage -- it used to print a note per stage, train from scratch and overwrite best_model.pth
    # although the user asked to resume
    resume_owner = None
    if isinstance(args.resume, str):
        resume_owner = T.checkpoint_stage(args.resume, config)
        stages = {"train_joint": ("joint",), "train_dehazing": ("low", "medium", "high"),
                  "train_all": ("low", "medium", "high", "joint")}.get(args.mode, ())
        if stages and resume_owner not in stages:
            raise SystemExit(f"--resume {args.resume} is a '{resume_owner}' checkpoint, but --mode {args.mode} runs only the "
                             f"stage(s) {', '.join(stages)}: nothing would resume from it (and training from scratch would "
                             "overwrite best_model.pth).  Pick the matching --mode, or drop --resume.")
    if args.mode == "train_classifier":
        # main.py:100-104 of the reference: train, then evaluate on the test split
        print("Training fog intensity classifier...")
        from training.train_classifier import evaluate_classifier, train_classifier
        classifier = train_classifier(config, epochs=args.epochs)
        evaluate_classifier(classifier, config)
    elif args.mode == "train_joint":
        T.train_joint_model(config, epochs=args.epochs, resume=resume_for("joint"))
    elif args.mode == "train_dehazing":
        for level in ("low", "medium", "high"):   # train_dehazing.py:216-232
            T.train_dehazing_model(config, level, epochs=args.epochs or 30, resume=resume_for(level))
    elif args.mode == "train_all":
        # main.py:121-139 of the reference: classifier -> dehazing branches -> joint -> evaluation.  Step 1 (stand-alone
        # classifier training) is not run by this mode (run --mode train_classifier first): the joint step fine-tunes the
        # classifier from whatever checkpoint `classifier.checkpoint_dir` holds, as train_joint.py:18-27 does when it is missing
        print("\n===== Step 1: fog-intensity classifier training is not run by train_all (--mode train_classifier): skipped =====")
        print("\n===== Step 2: Training Dehazing Models =====")
        for level in ("low", "medium", "high"):
            T.train_dehazing_model(config, level, epochs=args.epochs or 30, resume=resume_for(level))
        print("\n===== Step 3: Training Joint Model =====")
        T.train_joint_model(config, epochs=args.epochs, resume=resume_for("joint"))
        print("\n===== Step 4: Comprehensive Evaluation =====")
        T.run_comprehensive_evaluation(config)
    elif args.mode == "evaluate":
        # evaluate.py:464-540 (the reference first rewrites the checkpoint paths to a hard-coded experiment directory, main.py:143-145:
        # here the paths of the config are used as they are)
        T.run_comprehensive_evaluation(config)   # baseline branches, routed system, detector on hazy vs dehazed frames
    elif args.mode == "synthesize":
        from adam_dehaze_amd.data import synthesize_tree
        section = (config.get("dataset") or {}).get("synthetic_haze") or {}
        synthesize_tree(args.input, args.output, depth_dir=args.depth, seed=config["seed"], device=config.get("device", "cuda"),
                        nonuniform=(section.get("nonuniform") or True) if args.nonuniform else None,
                        chromatic=(section.get("chromatic") or True) if args.chromatic else None)
    elif args.mode == "demo" and args.input and args.fit_niqe:
        T.fit_niqe_model(config, args.input, args.fit_niqe)
    elif args.mode == "demo" and args.input:
        options = {}                                   # only the flags given: without any, the call is the plain one
        if args.target:
            options["target"] = args.target
        if args.self_ensemble:
            options["self_ensemble"] = args.self_ensemble
        if args.exif:
            options["exif"] = True
        if args.ms_ssim:
            options["ms_ssim"] = True
        if args.detect:
            options["detect"] = True
        if args.detect_threshold is not None:
            options["detect_threshold"] = args.detect_threshold
        if args.niqe:
            options["niqe"] = args.niqe
        if args.brisque_model:
            options["brisque_model"] = args.brisque_model
        if args.brisque_range:
            options["brisque_range"] = args.brisque_range
        T.run_demo(config, args.input, args.output, args.panels, **options)
    elif args.mode == "demo":
        # without --input: one synthetic batch through the router
        from adam_dehaze_amd.image_io import routing_records
        system = T.build_joint_system(config)
        system["router"].eval()
        batch = next(T.synthetic_loader(2, config["dataset"]["img_size"], 1, seed=config["seed"], device=config["device"]))
        with torch.no_grad():
            out, aux = system["router"](batch["hazy"])
        print("dehazed", tuple(out.shape), "weights", [r["weights"] for r in routing_records(aux)])
    else:
        raise SystemExit(f"mode '{args.mode}' is outside the hot path this build covers (see DESIGN.md section 7)")
    if world > 1:
        import torch.distributed as dist
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
