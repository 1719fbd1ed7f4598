from .trainer import (batch_processor, build_optimizer, change_input_variable, Runner, DataParallelShell,
                      StepLrUpdaterHook, train_mono)
from .env import init_dist, get_dist_info, set_random_seed, get_root_logger
from .checkpoint import save_checkpoint, load_checkpoint, weights_to_cpu
from .inference import (evaluate_depth, evaluate_depth_lidar, pose_between, chain_poses, odometry, pose_nets_from_checkpoint, chain_poses_device,
                        pair_transforms, odometry_device, evaluate_odometry, read_kitti_poses, write_kitti_poses, freeze, unfreeze)
from .perception import (Perceiver, Perception, VideoPerception, colorize_disp, layout_rgb, default_lut, quantiles,
                         disp_resize_depth, layout_classes, colorize)
from .stream import PerceptionStream, StreamFrame
from .bevmap import BevMap
from .depthbev import DepthBev, agreement_scores
from .bevobj import BevObjects
from .bevtrack import BevTracker
from .bevfilter import BevTrackFilter

__all__ = ["batch_processor", "train_mono", "build_optimizer", "change_input_variable", "Runner", "DataParallelShell", "init_dist",
           "get_dist_info", "set_random_seed", "get_root_logger", "StepLrUpdaterHook", "save_checkpoint", "load_checkpoint", "weights_to_cpu",
           "Perceiver", "Perception", "VideoPerception", "colorize_disp", "layout_rgb", "default_lut", "quantiles", "disp_resize_depth",
           "layout_classes", "colorize", "chain_poses_device", "pair_transforms", "odometry_device", "evaluate_odometry",
           "read_kitti_poses", "write_kitti_poses", "evaluate_depth_lidar", "freeze", "unfreeze", "PerceptionStream",
           "StreamFrame", "BevMap", "DepthBev", "agreement_scores", "BevObjects", "BevTracker", "BevTrackFilter"]
