// Test driver (CPU tier): replays scripts through node/VisibleRegion.mjs.  usage: node reveal_via_node.mjs <job.json>
// job: [{name, multiplier, sceneCenter, events: [{op: 'build', reset, update, finalBuild, distance} | {op: 'frames', mode, count, keep}]}]
// prints {name: [rows]}: after a build [centre x, y, z, ...state()], after every kept frame state().
import fs from 'fs';
import { VisibleRegion } from '../node/VisibleRegion.mjs';
const jobs = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const out = {};
for (const job of jobs) {
  const machine = new VisibleRegion(job.multiplier), rows = [];
  for (const ev of job.events) {
    if (ev.op === 'build') {
      if (ev.reset) machine.reset();
      machine.update(ev.update, [job.sceneCenter], ev.finalBuild, () => ev.distance);
      rows.push(machine.calculatedSceneCenter.concat(machine.state()));
    } else {
      const keep = new Set(ev.keep);
      for (let k = 0; k < ev.count; k++) {
        machine.updateFadeDistance(ev.mode);
        if (keep.has(k)) rows.push(machine.state());
      }
    }
  }
  out[job.name] = rows;
}
console.log(JSON.stringify(out));
