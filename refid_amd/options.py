"""YAML option files with the reference's keys (basicsr/utils/options.py:6-95)."""
from collections import OrderedDict
from os import path as osp

import yaml


def ordered_yaml():
    try:
        from yaml import CDumper as Dumper
        from yaml import CLoader as Loader
    except ImportError:
        from yaml import Dumper, Loader
    tag = yaml.resolver.BaseResolver.DEFAULT_MAPPING_TAG
    Dumper.add_representer(OrderedDict, lambda d, data: d.represent_dict(data.items()))
    Loader.add_constructor(tag, lambda l, node: OrderedDict(l.construct_pairs(node)))
    return Loader, Dumper


def parse(opt_path, is_train=True):
    """Same derived keys as the reference parser: is_train, datasets.*.phase/scale, path.*,
    debug-mode overrides for names containing 'debug' (options.py:31-95)."""
    with open(opt_path, mode="r") as f:
        Loader, _ = ordered_yaml()
        opt = yaml.load(f, Loader=Loader)
    opt["is_train"] = is_train
    if "datasets" in opt:
        for phase, dataset in opt["datasets"].items():
            phase = phase.split("_")[0]
            dataset["phase"] = phase
            if "scale" in opt:
                dataset["scale"] = opt["scale"]
            for key in ("dataroot_gt", "dataroot_lq"):
                if dataset.get(key) is not None:
                    dataset[key] = osp.expanduser(dataset[key])
    opt.setdefault("path", OrderedDict())
    for key, val in opt["path"].items():
        if val is not None and ("resume_state" in key or "pretrain_network" in key):
            opt["path"][key] = osp.expanduser(val)
    opt["path"]["root"] = opt["path"].get("root", osp.abspath(osp.join(__file__, osp.pardir, osp.pardir)))
    if is_train:
        root = osp.join(opt["path"]["root"], "experiments", opt["name"])
        opt["path"]["experiments_root"] = root
        opt["path"]["models"] = osp.join(root, "models")
        opt["path"]["training_states"] = osp.join(root, "training_states")
        opt["path"]["log"] = root
        opt["path"]["visualization"] = osp.join(root, "visualization")
        if "debug" in opt["name"]:
            if "val" in opt:
                opt["val"]["val_freq"] = 8
            opt.setdefault("logger", OrderedDict())
            opt["logger"]["print_freq"] = 1
            opt["logger"]["save_checkpoint_freq"] = 8
    else:
        root = osp.join(opt["path"]["root"], "results", opt["name"])
        opt["path"]["results_root"] = root
        opt["path"]["log"] = root
        opt["path"]["visualization"] = osp.join(root, "visualization")
    return opt


def shapes_from_dataset_opt(ds):
    """(T, img_chn) implied by a dataset block: image_npy_dataset.py:48,211-232 (blur-VFI,
    return_deblur_voxel) and image_sharp_npy_dataset.py:52 (sharp-VFI).  SURVEY.md 3.4."""
    m = int(ds.get("num_end_interpolation", 1))
    n = int(ds.get("num_inter_interpolation", 1))
    if ds.get("return_deblur_voxel", False):
        return 2 * m + n, 2 * 3 + 2 * (m - 1)
    return n, 6


def assembler_from_dataset_opt(ds, device=None):
    """``device_assemble: true`` in a dataset block selects batch assembly on the GPU: returns the
    ``refid_amd.data.DeviceBatchAssembler`` for the block's num_end_interpolation / num_inter_interpolation / gt_size
    / use_hflip / use_rot (hand it to ``CUDAPrefetcher(..., assemble=...)``; its ``draw(rng, H, W)`` draws a sample's crop and
    flips the way the reference does).  None when the key is absent or false.
    The layout follows the dataset class: the sharp-interpolation datasets (``*Sharp*``, image_sharp_npy_dataset.py) give
    lq (2,3,h,w), the blur datasets with ``return_deblur_voxel`` the 6+2(m-1)-channel lq.  A ``type`` containing
    ``SingleImage`` (GoProSingleImageEventDataset, data/Single_image_npy_dataset.py) gives ``layout='single'`` with the
    block's ``num_bins``: lq (3,h,w), gt (3,h,w), voxel (num_bins,h,w).  There ``norm_voxel`` counts as TRUE whatever the
    block says: the reference's __getitem__ normalises unconditionally (:187; the switch at :172-173 is commented out)."""
    if not ds.get("device_assemble", False):
        return None
    from ._lib import RefidHipError
    from .data import DeviceBatchAssembler
    if "singleimage" in str(ds.get("type", "")).lower():
        if "num_bins" not in ds:
            raise RefidHipError("device_assemble: the single-image dataset needs num_bins (Single_image_npy_dataset.py:48)")
        return DeviceBatchAssembler(layout="single", num_bins=int(ds["num_bins"]), norm_voxel=True,
                                    gt_size=ds.get("gt_size"), use_hflip=ds.get("use_hflip", False),
                                    use_rot=ds.get("use_rot", False), device=device)
    if not ds.get("one_voxel_flag", True):
        raise RefidHipError("device_assemble: the per-pair voxel mode (one_voxel_flag: false) is not supported")
    sharp = "sharp" in str(ds.get("type", "")).lower()
    if sharp and ds.get("return_deblur_voxel", False):
        raise RefidHipError("device_assemble: the sharp layout's zero-padded return_deblur_voxel "
                            "(image_sharp_npy_dataset.py:203-214) is not supported")
    if not sharp and not ds.get("return_deblur_voxel", False):
        raise RefidHipError("device_assemble: the blur datasets are supported with return_deblur_voxel: true only")
    # norm_voxel: accepted and ignored -- the reference discards voxel_norm's result (image_npy_dataset.py:206-208)
    return DeviceBatchAssembler(int(ds.get("num_end_interpolation", 1)), int(ds.get("num_inter_interpolation", 1)),
                                layout="sharp" if sharp else "blur", gt_size=ds.get("gt_size"),
                                use_hflip=ds.get("use_hflip", False), use_rot=ds.get("use_rot", False), device=device)
