"""`python -m fplx.nll_main train|test config.cfg` - the reference's `pymic_nll` entry (PyMIC/pymic/net_run_nll/nll_main.py:16-41):
parse + synchronize the .cfg, log to <ckpt_save_dir>/log_<stage>.txt, NLLMethodDict[nll_method](config, stage).run().
As fplx/ssl_main.py, a training stage is followed by the test stage with the best checkpoint and the evaluation reports - but
the test stage runs through the NLL agent too: a checkpoint holds the whole BiNet / TriNet (net1.*, net2.*, net3.*), and the
prediction is its eval-mode output."""
import logging
import os
import sys

from .config import parse_config, synchronize_config
from .net_run import eva_main
from .nll import nll_agent_class


def main(argv=None):
    argv = sys.argv if argv is None else argv
    if len(argv) < 3:
        print('Number of arguments should be 3. e.g.')
        print('   python -m fplx.nll_main train config.cfg')
        return 1
    stage, cfg_file = str(argv[1]), str(argv[2])
    config = synchronize_config(parse_config(cfg_file))
    log_dir = config['training']['ckpt_save_dir']
    os.makedirs(log_dir, exist_ok=True)
    logging.basicConfig(filename=log_dir + "/log_{0:}.txt".format(stage), level=logging.INFO, format='%(message)s',
                        force=True)
    task = config['dataset'].get('task_type', 'seg')
    if task != 'seg':
        raise ValueError("fplx.nll_main: only task_type = seg is built (got {0:})".format(task))
    config['network'].setdefault('num_domains', 1)
    agent_class = nll_agent_class(config['noisy_label_learning']['nll_method'])
    if stage == 'train':
        agent_class(config, stage).run()
    if 'testing' in config:
        config['testing'].setdefault('domian_label', 0)
        agent_class(config, 'test').run()
        return eva_main(config)
    return None


if __name__ == "__main__":
    r = main()
    sys.exit(r if isinstance(r, int) else 0)
