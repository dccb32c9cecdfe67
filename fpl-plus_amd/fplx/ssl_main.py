"""`python -m fplx.ssl_main train|test config.cfg` - the reference's `pymic_ssl` entry (PyMIC/pymic/net_run_ssl/ssl_main.py:23-44):
parse + synchronize the .cfg, log to <ckpt_save_dir>/log_<stage>.txt, SSLMethodDictAll[ssl_method](config, stage).run().
Otherwise as fplx/net_run.py: after a training stage the test stage runs with the student's best checkpoint (through the
supervised agent - a checkpoint holds the student only; CPS: through its own agent, the checkpoint holds the BiNet), then the evaluation reports are written."""
import logging
import os
import sys

from .agent import SegmentationAgent
from .config import parse_config, synchronize_config
from .net_run import eva_main
from .ssl import SSLCPS, ssl_agent_class_all


def main(argv=None):
    argv = sys.argv if argv is None else argv
    if len(argv) < 3:
        print('Number of arguments should be 3. e.g.')
        print('   python -m fplx.ssl_main train config.cfg')
        return 1
    stage, cfg_file = str(argv[1]), str(argv[2])
    config = synchronize_config(parse_config(cfg_file))
    log_dir = config['training']['ckpt_save_dir']
    os.makedirs(log_dir, exist_ok=True)
    logging.basicConfig(filename=log_dir + "/log_{0:}.txt".format(stage), level=logging.INFO, format='%(message)s',
                        force=True)
    task = config['dataset'].get('task_type', 'seg')
    if task != 'seg':
        raise ValueError("fplx.ssl_main: only task_type = seg is built (got {0:})".format(task))
    config['network'].setdefault('num_domains', 1)
    if stage == 'train':
        ssl_method = config['semi_supervised_learning']['ssl_method']
        agent = ssl_agent_class_all(ssl_method)(config, stage)
        agent.run()
    if 'testing' in config:
        config['testing'].setdefault('domian_label', 0)
        # a CPS checkpoint holds the whole BiNet (net1.*, net2.*): its test stage runs through the CPS agent, as fplx/nll_main.py
        cps = config.get('semi_supervised_learning', {}).get('ssl_method', None) == 'CPS'
        (SSLCPS if cps else SegmentationAgent)(config, 'test').run()
        return eva_main(config)
    return None


if __name__ == "__main__":
    r = main()
    sys.exit(r if isinstance(r, int) else 0)
