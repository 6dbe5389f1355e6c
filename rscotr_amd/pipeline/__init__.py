"""Device-side input path: the per-sample pipeline tail of the reference's dataset configs and the collate
step as HIP launches per batch, plus thin readers for the three datasets' on-disk layouts.

Reference pipelines (configs/_base_/cls/resisc_swin_224.py:7-39, configs/_base_/det/dior.py:11-20,
configs/_base_/seg/potsdam_IRRG_all.py:8-19):
    decode (host) -> [Resize / RandomResizedCrop] -> RandomCrop window (seg) -> RandomFlip -> [RandomRotate (seg)]
           -> [PhotoMetricDistortion] -> [RandomErasing] -> Normalize(mean, std, to_rgb) -> Pad
           -> ImageToTensor / DefaultFormatBundle -> collate
(bracketed: the optional stages; mmcls RandAugment sits between RandomFlip and RandomErasing in the cls pipeline).
Everything from the crop window on runs on the device; the host only draws the random decisions and uploads the raw bytes.

    resample   the integer resampling tables the host builds (cv2 bilinear, Pillow bicubic, nearest), cv2's bicubic remap weights
    randaug    RandAugment's configuration, draws, meta rows and warp tables
    autoaug    multi-scale Resize and mmdet AutoAugment (Resize / RandomCrop policies): draws, box chain, chain-launch tables
    rotate     mmseg RandomRotate: settings, draws, the rot rows and warp tables of the rotating launches
    collate    DeviceCollate (one host plan under five launch routes), the dataset configs' settings, the seg TTA collate
    config     build_collate: an mm* pipeline config -> a collate
    datasets   FolderClsDataset, CocoDetDataset, TileSegDataset with their evaluate / pre_eval, DeviceLoader"""
from .collate import (AUG_META, AUG_PARAMS, CLS_ERASING, IMG_NORM, PHOTOMETRIC, PM_BRIGHT, PM_CONTRAST, PM_CONTRAST_FIRST, PM_HUE,
                      PM_SAT, META, RANDOM_ERASING, RANDOM_RESIZED_CROP, SEG_TTA_MAX_VIEWS, DeviceCollate, SegTTACollate,
                      collate_for, eval_collate_for, plan_tta_views, train_collate_for)
from .config import build_collate
from .datasets import CocoDetDataset, DeviceLoader, FolderClsDataset, TileSegDataset
from .randaug import (RA_META, RA_OPS, RA_SIGNED, RA_STATS, RA_STATS_OPS, RA_WARPS, RAND_AUGMENT, RAND_INCREASING_POLICIES,
                      ra_draws, ra_meta_row, ra_slot_rows, ra_unsupported)
from .resample import (RESAMPLE_LINEAR, RESAMPLE_NEAREST, RESAMPLE_PIL, cubic_weight_table, rescale_size, scale_boxes)
