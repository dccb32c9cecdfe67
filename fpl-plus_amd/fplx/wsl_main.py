"""`python -m fplx.wsl_main train|test config.cfg` - the reference's `pymic_wsl` entry (PyMIC/pymic/net_run_wsl/wsl_main.py:22-43):
parse + synchronize the .cfg, log to <ckpt_save_dir>/log_<stage>.txt, WSLMethodDict[wsl_method](config, stage).run().
Otherwise as fplx/ssl_main.py: after a training stage the test stage runs with the best checkpoint through the supervised
agent (a checkpoint holds the student only), then the evaluation reports are written."""
import logging
import os
import sys

from .agent import SegmentationAgent
from .config import parse_config, synchronize_config
from .net_run import eva_main
from .wsl import wsl_agent_class


def main(argv=None):
    argv = sys.argv if argv is None else argv
    if len(argv) < 3:
        print('Number of arguments should be 3. e.g.')
        print('   python -m fplx.wsl_main train config.cfg')
        return 1
    stage, cfg_file = str(argv[1]), str(argv[2])
    config = synchronize_config(parse_config(cfg_file))
    log_dir = config['training']['ckpt_save_dir']
    os.makedirs(log_dir, exist_ok=True)
    logging.basicConfig(filename=log_dir + "/log_{0:}.txt".format(stage), level=logging.INFO, format='%(message)s',
                        force=True)
    task = config['dataset'].get('task_type', 'seg')
    if task != 'seg':
        raise ValueError("fplx.wsl_main: only task_type = seg is built (got {0:})".format(task))
    config['network'].setdefault('num_domains', 1)
    if stage == 'train':
        wsl_method = config['weakly_supervised_learning']['wsl_method']
        agent = wsl_agent_class(wsl_method)(config, stage)
        agent.run()
    if 'testing' in config:
        config['testing'].setdefault('domian_label', 0)
        SegmentationAgent(config, 'test').run()
        return eva_main(config)
    return None


if __name__ == "__main__":
    r = main()
    sys.exit(r if isinstance(r, int) else 0)
