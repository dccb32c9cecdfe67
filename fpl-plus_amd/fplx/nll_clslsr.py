"""`python -m fplx.nll_clslsr config.cfg` - the reference's `pymic_nll` confidence tool (PyMIC/pymic/net_run_nll/nll_clslsr.py:
48-204, CLSLSR: confident learning + spatial label smoothing, Zhang et al., MICCAI 2020): predict every TRAINING case with a
trained network, find the suspect labels of the whole set with confident learning (fplx.confident), write one mask per case to
<root_dir>/slsr_conf/ and a csv `<train_csv minus .csv>_clslsr.csv` with the columns image, pixel_weight, label.  The second
stage is the ordinary supervised run with loss_type = SLSRLoss on that csv.

As in the reference: valid_transform on train_csv, the checkpoint of [testing] ckpt_mode / ckpt_name, evaluation mode or
test_time_dropout, the Inferer, the inverse transforms of the prediction.  On the device: every case's logits go as C planes
into ONE planar buffer [C][M_total] and its labels into [M_total]; one get_confident_map over the whole set; the mask is cut
back per case.

3D, on purpose: the reference hard-codes 2D 256 x 256 PNGs (its two swapaxes are right for [N, C, H, W] only); fplx is 3D, so
volumes in and NIfTI out, uint8 * 255 with the label file's header.  The reference inverse-transforms the prediction but leaves
the label transformed; here the prediction is brought back to the stored label's grid and compared with the STORED label, and a
shape disagreement raises.  Refused: domain-specific-BatchNorm networks, torch.distributed groups, networks with several
outputs (deep supervision) and ckpt_mode = 3 (the reference returns without a map there)."""
import logging
import os
import sys

import pandas as pd
import torch
import torch.nn as nn

from . import confident
from .agent import SegmentationAgent
from .config import parse_config, synchronize_config
from .dataset import NiftyDataset, collate
from .infer import Inferer
from .nifti import save_array_as_nifty_volume
from .transform import TransformDict, Compose

_DSBN_NAMES = ('UNet2D5_dsbn', 'UNet3D_dsbn')
MAX_VOXELS = 1 << 31


class NLLCLSLSR(SegmentationAgent):
    def __init__(self, config, stage='test'):
        net_type = config.get('network', {}).get('net_type', None)
        if net_type in _DSBN_NAMES:
            raise ValueError("fplx nll_clslsr: {0:} is a domain-specific-BatchNorm network; the confidence tool derives from "
                             "net_run/agent_seg.py and runs UNet2D5 / UNet3D only".format(net_type))
        if config.get('network', {}).get('deep_supervise', False):
            raise ValueError("fplx nll_clslsr: a network with several outputs (deep_supervise) has no single prediction to "
                             "judge the labels with")
        if config.get('testing', {}).get('ckpt_mode', None) == 3:
            raise ValueError("fplx nll_clslsr: ckpt_mode = 3 (an ensemble of checkpoints) gives no confidence map - the reference "
                             "returns without one; name one checkpoint")
        config['network'].setdefault('num_domains', 1)
        super(NLLCLSLSR, self).__init__(config, stage)
        if self.distributed:
            raise ValueError("fplx nll_clslsr: the confidence tool runs in a single process (no torch.distributed group): the map "
                             "is one statistic over the whole training set")

    def infer_with_cl(self):
        """-> {label file name: uint8 mask [D, H, W] on the device, 1 = suspect}; writes <root_dir>/slsr_conf/<name>"""
        cfg = self.config['testing']
        ckpt_name = self.get_checkpoint_name()
        if isinstance(ckpt_name, (tuple, list)):
            raise ValueError("ckpt_mode should be 3 if ckpt_name is a list")
        self.net.to(self.device)
        if cfg.get('evaluation_mode', True):
            self.net.eval()
            if cfg.get('test_time_dropout', False):
                def test_time_dropout(m):
                    if type(m) == nn.Dropout:
                        logging.info('dropout layer')
                        m.train()
                self.net.apply(test_time_dropout)
        checkpoint = torch.load(ckpt_name, map_location=self.device, weights_only=False)
        self.net.load_state_dict(checkpoint['model_state_dict'])
        class_num = self.config['network']['class_num']
        if self.inferer is None:
            infer_cfg = dict(cfg)
            infer_cfg['class_num'] = class_num
            self.inferer = Inferer(infer_cfg)
        ds = self.test_set
        if not isinstance(ds, NiftyDataset) or not ds.with_label:
            raise ValueError("fplx nll_clslsr: the confidence tool needs a NiftyDataset with labels")
        label_col = list(ds.csv_items.keys()).index('label')
        # the stored labels first: they size the one buffer
        labels, offsets, total = [], [0], 0
        for idx in range(len(ds)):
            lab = ds.__getlabel__(idx)
            if lab.dim() != 4 or lab.shape[0] != 1:
                raise ValueError("fplx nll_clslsr: label {0:} is not one 3D volume".format(ds.csv_items.iloc[idx, label_col]))
            total += lab.numel()
            if total >= MAX_VOXELS:
                raise ValueError("fplx nll_clslsr: the training set has 2^31 voxels or more after {0:} cases; only the first {1:} "
                                 "fit into one confident-learning run (select_kth's bound)".format(idx + 1, idx))
            labels.append(lab)
            offsets.append(total)
        if total == 0:
            raise ValueError("fplx nll_clslsr: the training set is empty")
        logits = torch.empty((class_num, total), dtype=torch.float32, device=self.device)
        gt = torch.empty(total, dtype=torch.uint8, device=self.device)
        dl0 = cfg.get('domian_label', 0)
        with torch.no_grad():
            for idx in range(len(ds)):
                data = collate([ds[idx]])
                images = self.convert_tensor_type(data['image']).to(self.device)
                dl = dl0 * torch.ones(images.shape[0], dtype=torch.long)
                pred = self.inferer.run(self.net, images, dl)
                if isinstance(pred, (tuple, list)):
                    raise ValueError("fplx nll_clslsr: the network returned several outputs")
                data['predict'] = pred
                for transform in self.transform_list[::-1]:
                    if transform.inverse:
                        data = transform.inverse_transform_for_prediction(data)
                pred = data['predict']
                lab = labels[idx]
                if tuple(pred.shape) != (1, class_num) + tuple(lab.shape[1:]):
                    raise ValueError("fplx nll_clslsr: the prediction of {0:} is {1:} after the inverse transforms, its stored label "
                                     "{2:}".format(data['names'][0], tuple(pred.shape), tuple(lab.shape)))
                logits[:, offsets[idx]:offsets[idx + 1]].copy_(pred[0].reshape(class_num, -1))
                gt[offsets[idx]:offsets[idx + 1]].copy_(lab.reshape(-1))
        self.cl_logits, self.cl_labels, self.cl_offsets = logits, gt, offsets
        cl_type = self.config.get('noisy_label_learning', {}).get('clslsr_cl_type', 'both')
        conf = confident.get_confident_map(gt, logits, cl_type, planar=True)
        root_dir = self.config['dataset']['root_dir']
        save_dir = root_dir + "/slsr_conf"
        os.makedirs(save_dir, exist_ok=True)
        out = {}
        for idx in range(len(ds)):
            lab_name = str(ds.csv_items.iloc[idx, label_col])
            filename = lab_name.split('/')[-1]
            m = conf[offsets[idx]:offsets[idx + 1]].reshape(labels[idx].shape[1:])
            out[filename] = m
            save_array_as_nifty_volume((m * 255).cpu().numpy(), os.path.join(save_dir, filename), root_dir + '/' + lab_name)
        return out


def get_confidence_map(argv=None):
    """nll_clslsr.py:149-204"""
    argv = sys.argv if argv is None else argv
    if len(argv) < 2:
        print('Number of arguments should be 2. e.g.')
        print('   python -m fplx.nll_clslsr config.cfg')
        return 1
    config = synchronize_config(parse_config(str(argv[1])))
    ds = config['dataset']
    transform_names = ds['valid_transform']
    transform_list, data_transform = [], None
    if transform_names is not None and len(transform_names) > 0:
        ds['task'] = 'segmentation'
        for name in transform_names:
            if name not in TransformDict:
                raise ValueError("Undefined transform {0:}".format(name))
            transform_list.append(TransformDict[name](ds))
        data_transform = Compose(transform_list)
    csv_file = ds['train_csv']
    agent = NLLCLSLSR(config, 'test')
    dataset = NiftyDataset(root_dir=ds['root_dir'], csv_file=csv_file, modal_num=ds.get('modal_num', 1), with_label=True,
                           transform=data_transform, device=agent.device, cache=False)
    agent.set_datasets(None, None, dataset)
    agent.transform_list = transform_list
    agent.create_dataset()
    agent.create_network()
    agent.infer_with_cl()
    # the training csv of the second stage
    df_train = pd.read_csv(csv_file)
    pixel_weight = ["slsr_conf/" + str(name).split('/')[-1] for name in df_train["label"]]
    df_cl = pd.DataFrame.from_dict({"image": df_train["image"], "pixel_weight": pixel_weight, "label": df_train["label"]})
    df_cl.to_csv(csv_file.replace(".csv", "_clslsr.csv"), index=False)
    return agent


if __name__ == "__main__":
    r = get_confidence_map()
    sys.exit(r if isinstance(r, int) else 0)
